"""Writes the tests/golden/oracle/bal_*.npz and baltrain_*.npz records: the float64 CPU oracle's outputs for the seeded
cases of the balanced step (tests/balanced_reference.py, tests/balanced_training.py).  The companion of
make_inverse_oracle_cache.py; run in the build container (no GPU needed):

    python tests/golden/make_balanced_oracle_cache.py [-j 4] [-k substring]

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
    import balanced_reference as BR
    import balanced_training as BT
    return [("step", c, "") for c in BR.CASES] + [("train", c, h) for c in BT.TRAIN_CASES for h in ("", "hold")]


def cost(job):
    import balanced_reference as BR
    if job[0] == "train":
        return 10 ** 9
    ans, n, L, enc, B_res, n_ic, n_bc = BR.CASES[job[1]]
    return 2 ** n * L * (6 * n * B_res + n_ic + n_bc)


def run(job):
    import torch
    torch.set_num_threads(2)
    import balanced_reference as BR
    import balanced_training as BT
    if job[0] == "step":
        BR.class_reference(job[1])
    else:
        BT.training_reference(job[1], hold=job[2] == "hold")
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
