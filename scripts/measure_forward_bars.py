"""Measure the fp64 oracle and the kernels' scheme (tests/host_emul) against the long-double oracle on the case set of
tests/test_forward_long_double.py, write tests/golden/fdem_ld_bars.json and print the table.  CPU only, no arguments.

Per cell (system, altitude band, tensor id, quantity) two bars, both as a share of the present parity bar
(|x - ld| / (ATOL + RTOL |ld|), tests/conftest.py):
  reference_bar  the fp64 oracle's largest distance from long double, at most 1;
  scheme_bar     four times the host emulation's largest distance, at most reference_bar and at least 16 * 2^-11 of the
                 oracle's distance (the long-double value's own rounding).
The emulation must be built from the headers the bars are to pin (the parent commit's, when a change to them is under test).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_forward_long_double as t  # noqa: E402


def main():
    cells = {}
    meas = {}
    for name in t.SYSTEMS:
        m = t.measure(name)
        meas.update(m)
        cells.update(t.bars_from(m))
    doc = {
        "unit": "share of the present bar: |x - long double| / (atol + rtol |long double|); *_abs in ppm (pred, J) or plain (chi2, logL)",
        "present_bar": {"pred": [t.PRED_ATOL, t.PRED_RTOL], "J": [t.PRED_ATOL, t.PRED_RTOL], "J_exact": [t.PRED_ATOL, t.PRED_RTOL],
                        "chi2": [t.LIKE_ATOL, t.LIKE_RTOL], "logL": [t.LIKE_ATOL, t.LIKE_RTOL]},
        "seed": t.SEED,
        "cells": {k: {w: float("%.6g" % v) for w, v in cells[k].items()} for k in sorted(cells)},
    }
    with open(t.BARS_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("| cell | fp64 oracle | scheme | reference_bar | scheme_bar | oracle abs | scheme abs |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(cells):
        print("| %s | %.3g | %.3g | %.3g | %.3g | %.3g | %.3g |" % (
            k, meas[k]["oracle"], meas[k]["scheme"], cells[k]["reference_bar"], cells[k]["scheme_bar"],
            meas[k]["oracle_abs"], meas[k]["scheme_abs"]))
    above = [v["scheme_bar"] for k, v in cells.items() if k.endswith("/pred") and "/0.5-3m/" not in k]
    print("largest pred scheme_bar above 3 m: %.3g (condition: <= 0.1)" % max(above))


if __name__ == "__main__":
    main()
