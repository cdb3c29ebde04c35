"""Record tests/golden/convt_plan.json over the shape grid of tests/test_convt_plan_host.py, in full
for the default tune state and as a SHA-256 for each single-key state. Needs a built library, no GPU.
Two steps, from the repo root:

    python tests/golden/record_convt_plan.py sizes --lib path/to/libpis.so
        pis_convt2x2_wgrad_ws and pis_debug_convt2x2_wgrad_tile_splits from the library of the
        commit before the planner (the reference); writes the file without the algorithm tables

    python tests/golden/record_convt_plan.py algos
        pis_debug_convt2x2_algo from this tree's library, added to the file; only after
        tests/test_convt_dispatch_gpu.py has passed with this library on the MI355X
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_convt_plan_host as t  # noqa: E402
from physics_informed_image_segmentation_amd import _hip  # noqa: E402


def load(path):
    """The library by path, binding only what this recorder calls (an older library lacks newer symbols)."""
    import torch  # noqa: F401  (its HIP runtime is the one the library binds to)
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.pis_convt2x2_wgrad_ws.restype = ctypes.c_size_t
    return lib


def tables(lib, fn):
    sha = {}
    for state in t.STATES:
        with t.tuned(lib, state):
            sha[state] = t.digest(fn(lib))
    return fn(lib), sha


def write(doc):
    with open(t.GOLDEN, "w") as f:
        f.write("{\n")
        for k in ("header", "size_columns", "algo_columns", "sizes_sha256", "algos_sha256"):
            f.write(' %s: %s,\n' % (json.dumps(k), json.dumps(doc[k], indent=1)))
        for k in ("sizes", "algos"):
            f.write(' "%s": [\n' % k + ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc[k]))
            f.write("\n ]%s\n" % ("," if k == "sizes" else ""))
        f.write("}\n")
    print("wrote", t.GOLDEN, os.path.getsize(t.GOLDEN), "bytes")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "sizes":
        lib = load(sys.argv[sys.argv.index("--lib") + 1]) if "--lib" in sys.argv else _hip.lib()
        rows, sha = tables(lib, t.sizes)
        write({"header": "sizes: from the library of the commit before csrc/convt_plan.hip existed. algos: not recorded yet.",
               "size_columns": list(t.SIZE_COLUMNS), "algo_columns": list(t.ALGO_COLUMNS), "sizes_sha256": sha,
               "algos_sha256": {}, "sizes": rows, "algos": []})
    elif what == "algos":
        with open(t.GOLDEN) as f:
            doc = json.load(f)
        doc["algos"], doc["algos_sha256"] = tables(_hip.lib(), t.algos)
        doc["header"] = ("sizes: from the library of the commit before csrc/convt_plan.hip existed. algos: from the "
                         "planner, recorded after every digest of tests/golden/convt_dispatch.json (recorded at that "
                         "same earlier commit) had matched on the MI355X.")
        write(doc)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
