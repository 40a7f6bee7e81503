#!/usr/bin/env python
"""What the REFERENCE wrote and read for tests/test_hdf5_file.py, recorded as fixtures.  Needs the reference (REF of make_golden.py) and an
interpreter that has the real h5py and can import it (test_hdf5_file.CHECKER; GBP_H5PY_PYTHON names one):
    python tests/golden/make_reference_records.py
  reference_<kind>.h5.gz               the container the reference's own createHdf / writeHdf wrote into a real h5py.File
                                       (tests/ref_writes_h5.py), kind = resolve / skytem / tempest, after the iterations of
                                       test_hdf5_file.REFERENCE_RUN_ITERATIONS
  reference_reads_ours.json            what the reference's readers returned for sounding 1 of the seeded container this package writes
                                       (tests/ref_reads_h5.py on test_hdf5_file._seeded_container)
  reference_reads_device_survey.json   the same readers on soundings 0 and 7 of device_survey_0.0.h5"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import test_hdf5_file as T   # noqa: E402

assert T.CHECKER, "no interpreter with the real h5py"
ENV = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "PYTHONHOME")}
d = tempfile.mkdtemp()


def read(path, index):
    out = os.path.join(d, "read.json")
    subprocess.run([T.CHECKER, os.path.join(ROOT, "tests", "ref_reads_h5.py"), path, str(index), out], check=True, env=ENV, timeout=900)
    return json.load(open(out))


try:
    for kind, n_run in T.REFERENCE_RUN_ITERATIONS.items():
        ref = os.path.join(d, "reference.h5")
        subprocess.run([T.CHECKER, os.path.join(ROOT, "tests", "ref_writes_h5.py"), ref, kind, str(n_run)], check=True, env=ENV, cwd=d, timeout=1800)
        with open(ref, "rb") as src, gzip.GzipFile(os.path.join(HERE, "reference_%s.h5.gz" % kind), "wb", compresslevel=9, mtime=0) as dst:
            shutil.copyfileobj(src, dst)
    ours = os.path.join(d, "0.0.h5")
    T._seeded_container(ours)
    json.dump(read(ours, 1), open(os.path.join(HERE, "reference_reads_ours.json"), "w"), sort_keys=True)
    json.dump({str(i): read(os.path.join(HERE, "device_survey_0.0.h5"), i) for i in (0, 7)},
              open(os.path.join(HERE, "reference_reads_device_survey.json"), "w"), sort_keys=True)
finally:
    shutil.rmtree(d, ignore_errors=True)
for f in sorted(os.listdir(HERE)):
    if f.startswith("reference_"):
        print(f, os.path.getsize(os.path.join(HERE, f)))
