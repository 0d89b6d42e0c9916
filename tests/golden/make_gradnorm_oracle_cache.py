"""Writes the tests/golden/oracle/gradnorm_*.npz and gradnormtrain_*.npz records: the float64 CPU oracle's outputs for the
seeded cases of the gradient-norm step (tests/gradnorm_reference.py).  The companion of make_causal_oracle_cache.py; run
in the build container (no GPU needed):

    python tests/golden/make_gradnorm_oracle_cache.py [-j 4] [-k substring]

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
    import gradnorm_reference as GR
    return [("step", c) for c in GR.STEP_CASES] + [("train", ""), ("train", "unit")]


def cost(job):
    import gradnorm_reference as GR
    return 2 ** GR.STEP_CASES[job[1]][2] if job[0] == "step" else 2 ** 5


def run(job):
    import torch
    torch.set_num_threads(2)
    import gradnorm_reference as GR
    if job[0] == "step":
        kind, ans, n, L, B_res, n_ic, n_bc = GR.STEP_CASES[job[1]]
        rec = GR.step_reference(job[1])
        _, st, _ = GR.expected_step(rec, n_ic, n_bc)
        return f"{job[1]}: m_r {st['m_r']:.4g} a_bc {st['a_bc']:.4g} a_ic {st['a_ic']:.4g} lam {st['lam_bc']:.4g} {st['lam_ic']:.4g}"
    out = GR.training_reference(unit=job[1] == "unit")
    return f"train {job[1]}: loss {out['loss'].round(4).tolist()} lam_bc {out['hist'][:, 0].round(3).tolist()} " \
        f"lam_ic {out['hist'][:, 1].round(3).tolist()}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=3)
    ap.add_argument("-k", default="")
    a = ap.parse_args()
    todo = sorted((j for j in jobs() if a.k in " ".join(j)), key=lambda j: -cost(j))
    with ProcessPoolExecutor(max_workers=a.j) as ex:
        for msg in ex.map(run, todo):
            print("done:", msg, flush=True)
