"""Writes the float64 records of the ensemble step's cases (tests/ensemble_reference.py) into tests/golden/oracle/, one per
case and member, the way make_oracle_cache.py writes the other records; no GPU needed:

    python tests/golden/make_ensemble_oracle.py [-k substring of a case id]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", default="", help="substring of a case id (cascade4, alternate5, ...)")
    a = ap.parse_args()
    os.environ["QC_WRITE_ORACLE_CACHE"] = "1"
    import ensemble_reference as ER
    for job in ER.oracle_jobs():
        if a.k in job.case:
            out = job.get()
            print("done:", job.key, ", ".join(f"{k} {v.shape}" for k, v in out.items()), flush=True)
