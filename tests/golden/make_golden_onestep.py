"""Writes tests/golden/f9_onestep.npz: the lanes of the one-step tests and what tests/onestep_ref.py expects of them at
np.longdouble (tests/onestep_cases.py build_fixture).  It holds recorded results of this project's own reference.

    python tests/golden/make_golden_onestep.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import onestep_cases as K  # noqa: E402

if __name__ == "__main__":
    fx = K.build_fixture()
    path = os.path.join(HERE, "f9_onestep.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes; redraws per stratum", fx["redraws"].tolist(), "E", fx["E"].tolist())
    print(dict(zip(fx["census_keys"].tolist(), fx["census"].tolist())))
