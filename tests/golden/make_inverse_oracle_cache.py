"""Writes the tests/golden/oracle/inv_*.npz and invtrain_*.npz records: the float64 CPU oracle's outputs for the seeded
cases of the inverse step (tests/inverse_reference.py, tests/inverse_training.py).  The companion of
make_coef_oracle_cache.py; run in the build container (no GPU needed):

    python tests/golden/make_inverse_oracle_cache.py [-j 4] [-k substring]

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
    import inverse_reference as IR
    import inverse_training as IT
    return [("step",) + j for j in IR.oracle_jobs()] + [("uniform_c3", "reg_cascade4", "")] + \
        [("train", c, h) for c in IT.TRAIN_CASES for h in ("", "hold")] + [("recover", "cascade2", "")]


def cost(job):
    import inverse_reference as IR
    if job[0] in ("train", "recover"):
        return 10 ** 9
    ans, n, L, enc, B_res, n_ic, n_bc = IR.CASES[job[1]]
    return 2 ** n * L * (6 * n * B_res + n_ic + n_bc)


def run(job):
    import torch
    torch.set_num_threads(2)
    import inverse_reference as IR
    import inverse_training as IT
    if job[0] == "step":
        IR.case_reference(job[1], job[2])
    elif job[0] == "uniform_c3":
        IR.uniform_c3_reference(job[1])
    elif job[0] == "train":
        IT.training_reference(job[1], hold=job[2] == "hold")
    else:
        IT.recovery_reference()
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
