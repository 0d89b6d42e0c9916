"""Writes the tests/golden/oracle/sys_*.npz and systrain_*.npz records: the float64 CPU oracle's outputs for the seeded
cases of the system step (tests/system_reference.py, tests/system_training.py).  The companion of
make_coef_oracle_cache.py; run in the build container (no GPU needed):

    python tests/golden/make_system_oracle_cache.py [-j 4] [-k substring]

It calls the SAME functions the tests call (conftest.cached_oracle with QC_WRITE_ORACLE_CACHE=1); the tests check the
inputs' digest before they trust a record.  The records are data (arrays) from this repository's own oracle/ package."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
os.environ["QC_WRITE_ORACLE_CACHE"] = "1"


def jobs():
    import system_reference as S
    return [("step",) + j for j in S.oracle_jobs()] + [("train", "cascade4", "")]


def cost(job):
    import system_reference as S
    if job[0] == "train":
        return 10 ** 9
    ans, n, L, enc, B_res, n_ic, n_bc, K = S.CASES[job[1]]
    return 2 ** n * L * (6 * n * B_res + n_ic + n_bc)


def run(job):
    import torch
    torch.set_num_threads(2)
    if job[0] == "step":
        import system_reference as S
        S.case_reference(job[1], job[2])
    else:
        import system_training as ST
        ST.training_reference()
    return " ".join(job)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=3)
    ap.add_argument("-k", default="")
    a = ap.parse_args()
    todo = sorted((j for j in jobs() if a.k in " ".join(j)), key=lambda j: -cost(j))
    with ProcessPoolExecutor(max_workers=a.j) as ex:
        for msg in ex.map(run, todo):
            print("done:", msg, flush=True)
