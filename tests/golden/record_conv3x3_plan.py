"""Record tests/golden/conv3x3_plan.json: what the 3x3-conv size and format queries answer over
the shape grid of tests/test_conv3x3_plan_host.py, in full for the default tune state and as a
SHA-256 for each single-key state. Needs the built library, no GPU. Run from the repo root, at
the commit whose decisions are the reference:

    python tests/golden/record_conv3x3_plan.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_conv3x3_plan_host as t  # noqa: E402
from physics_informed_image_segmentation_amd import _hip  # noqa: E402


def main():
    lib = _hip.lib()
    default = t.table(lib)
    sha = {}
    for state in t.STATES:
        with t.tuned(lib, state):
            rows = t.table(lib)
        sha[state] = t.digest(rows)
        print(f"{state}: {sum(a != b for a, b in zip(rows, default))} of {len(rows)} rows differ from the default")
    with open(t.GOLDEN, "w") as f:
        f.write('{"columns": %s,\n "sha256": %s,\n "default": [\n' % (json.dumps(list(t.COLUMNS)), json.dumps(sha, indent=1)))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in default))
        f.write("\n]}\n")
    print("wrote", t.GOLDEN, os.path.getsize(t.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
