"""Writes tests/golden/step_descriptors.json: the records every kind of fused step hands to the library (QcStepDesc and
its side records, pointers as null / the name of the tensor they address), for the cases of
tests/test_gpu_step_descriptors.py.  The companion of make_oracle_cache.py, but it needs a GPU: the
constructors allocate on the device and size the step workspace through the library.

    python tests/golden/make_step_descriptor_golden.py [-o FILE]

It calls the SAME function the tests call (test_gpu_step_descriptors.describe), which uses the public constructors only.
The committed file was recorded at the commit before the step classes were put on one base class; re-record it only with
a change that is MEANT to alter a record, from the parent of that change.  The record is data: hex strings and names."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=os.path.join(HERE, "step_descriptors.json"))
    a = ap.parse_args()
    import torch

    import test_gpu_step_descriptors as SD
    circ = SD._circuit(torch.device("cuda", 0))
    out = {}
    for kind in SD.KINDS:
        for case in SD.cases(kind):
            out[SD.key(kind, *case)], _ = SD.describe(kind, circ, *case)
            print("done:", SD.key(kind, *case), flush=True)
    with open(a.o, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(out)} steps to {a.o}")
