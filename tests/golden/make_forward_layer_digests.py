"""Records tests/golden/forward_layer_digests.json (tests/test_forward_bits_layers.py) on a GPU:
    python tests/golden/make_forward_layer_digests.py [LIBRARY.so] [OUT.json]
LIBRARY.so: the build whose outputs are recorded (default: the package's own library).  The committed record was made with the
library of the commit before the layer records of forward_passes_1f."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import geobipy_amd._lib as _lib  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "forward_layer_digests.json")

import test_forward_bits_layers  # noqa: E402

rec = test_forward_bits_layers.record()
with open(out, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out, len(rec), "cases with", _lib.LIB_PATH)
