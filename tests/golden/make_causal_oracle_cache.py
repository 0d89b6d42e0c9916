"""Writes the tests/golden/oracle/causal_*.npz and causaltrain_*.npz records: the float64 CPU oracle's outputs for the
seeded cases of the causal step (tests/causal_reference.py).  The companion of make_balanced_oracle_cache.py; run in the
build container (no GPU needed):

    python tests/golden/make_causal_oracle_cache.py [-j 4] [-k substring]

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
    import causal_reference as CR
    return [("hbm", "", "", "")] + [("train", c, k, u) for c in CR.TRAIN_CASES for k in CR.CONFIGS for u in ("", "unit")]


def cost(job):
    import causal_reference as CR
    if job[0] == "hbm":
        return 10 ** 9
    return 2 ** CR.TRAIN_CASES[job[1]][1] * CR.CONFIGS[job[2]][0]


def run(job):
    import torch
    torch.set_num_threads(2)
    import causal_reference as CR
    if job[0] == "hbm":
        CR.hbm_reference()
    else:
        out = CR.training_reference(job[1], job[2], unit=job[3] == "unit")
        return " ".join(job) + f" | W_last of step 1: {out['W'][0, -1]:.4f}, raised: {out['raised'].astype(int).tolist()}, " \
            f"W_last: {out['W'][:, -1].round(4).tolist()}"
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
