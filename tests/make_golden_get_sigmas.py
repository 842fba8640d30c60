"""Writes tests/golden/get_sigmas_rf.npz from the reference's own src/duwu/sampling/get_sigmas.py (numpy only, loaded by path):

    python tests/make_golden_get_sigmas.py <reference checkout>

``cases`` holds one row (num_steps, max_sigma, min_sigma, rho) per case; ``<disc>_<row>`` is get_sigmas_for_rf's float64 result
for the time discretisation ``disc`` (uniform_time ignores rho).  No test imports this script."""
import functools
import importlib.util
import os
import sys

import numpy as np

CASES = [(4, 14.6146, 0.0, 10.0), (16, 14.6146, 0.03, 10.0), (24, 80.0, 0.002, 7.0), (1, 14.6146, 0.0, 10.0), (8, 1.0, 0.0, 3.0),
         (24, 14.6146, 0.0, 10.0)]
DISCS = ("uniform_time", "sigmoid_time", "sigmoid_time_scale")

if __name__ == "__main__":
    path = os.path.join(sys.argv[1], "src", "duwu", "sampling", "get_sigmas.py")
    spec = importlib.util.spec_from_file_location("reference_get_sigmas", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"cases": np.asarray(CASES, dtype=np.float64)}
    for i, (steps, smax, smin, rho) in enumerate(CASES):
        for disc in DISCS:
            f = getattr(ref, disc)
            f = f if disc == "uniform_time" else functools.partial(f, rho=rho)
            out[f"{disc}_{i}"] = np.asarray(ref.get_sigmas_for_rf(steps, smax, smin, f), dtype=np.float64)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "get_sigmas_rf.npz")
    np.savez(dst, **out)
    print(dst, len(out) - 1, "arrays")
