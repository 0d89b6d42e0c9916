"""Writes the tests/golden/oracle/lbfgs_*.npz records: the float64 replays of the Adam -> L-BFGS runs of
tests/lbfgs_training.py (the cases of tests/test_gpu_lbfgs_train.py and the usefulness comparison).  The companion of
make_oracle_cache.py; run in the build container (no GPU needed):

    python tests/golden/make_lbfgs_oracle_cache.py [-k substring]

It calls the SAME functions the tests call (conftest.cached_oracle with QC_WRITE_ORACLE_CACHE=1); the tests check the
inputs' digest before they trust a record.  The replays assert their own conditions while they run: the Armijo slack at
every trial, at least one rejected trial, and a factor >= 2 between Adam alone and Adam -> L-BFGS.  The records are data
(arrays) from this repository's own oracle/ package."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
os.environ["QC_WRITE_ORACLE_CACHE"] = "1"


if __name__ == "__main__":
    import lbfgs_training as LT
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", default="")
    a = ap.parse_args()
    for case in LT.CASES:
        if a.k in case:
            r = LT.training_reference(case)
            print("done:", case, "accepted", r["accepted"].tolist(), flush=True)
    if a.k in "usefulness":
        r = LT.usefulness_reference()
        print("done: usefulness", {k: float(v[0]) for k, v in r.items()}, flush=True)
