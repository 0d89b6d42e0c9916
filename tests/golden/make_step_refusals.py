"""Records ``step_refusals.json``: the return code of every row of tests/step_refusal_cases.py, as the library built from
the commit BEFORE a change of the step's host code answers it.  Run where no GPU is visible::

    QC_LIB=<libqcpinn_hip.so of that commit> python tests/golden/make_step_refusals.py

(without QC_LIB: the library of this tree).  A row goes into the table only as a refusal (QC_ERR_ARG, QC_ERR_UNSUPPORTED)
or, for the baseline of an entry point, as QC_OK; anything else (a HIP error: something tried to run) stops the recording.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch                                 # noqa: E402

from conftest import pkg                     # noqa: E402
import step_refusal_cases as S               # noqa: E402


def main():
    if torch.cuda.is_available():
        sys.exit("a GPU is visible: the baseline rows would run; record where there is none")
    table = S.evaluate(pkg("hip.lib").load())
    bad = [r for r in table if r["code"] not in ((S.OK,) if not r["faults"] else (S.ERR_ARG, S.ERR_UNSUPPORTED))]
    if bad:
        sys.exit("not rows of a refusal table:\n" + "\n".join(map(str, bad)))
    with open(os.path.join(HERE, "step_refusals.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "rows;", sum(r["code"] == S.ERR_UNSUPPORTED for r in table), "QC_ERR_UNSUPPORTED,",
          sum(r["code"] == S.OK for r in table), "QC_OK")


if __name__ == "__main__":
    main()
