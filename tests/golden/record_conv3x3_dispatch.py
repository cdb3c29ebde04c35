"""Record tests/golden/conv3x3_dispatch.json on the MI355X: per case of
tests/test_conv3x3_dispatch_gpu.py the filter formats, the launch-hook names in order and the
SHA-256 of every output. Every case runs twice; a case whose two runs differ is reported and the
file is not written. Run from the repo root, at the commit whose kernels are the reference:

    python tests/golden/record_conv3x3_dispatch.py [--lib another/libpis.so] [--out another/file.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_conv3x3_dispatch_gpu as t  # noqa: E402
from physics_informed_image_segmentation_amd import _hip  # noqa: E402


def main():
    if "--lib" in sys.argv:
        _hip.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else t.GOLDEN
    lib = _hip.lib()
    out, bad = {}, []
    for name in t.CASES:
        a, b = t.run_case(lib, name), t.run_case(lib, name)
        print(name, json.dumps(a), flush=True)
        if a != b:
            bad.append(name)
            print(f"  NOT REPEATABLE: second run {json.dumps(b)}", flush=True)
        try:
            t.check_path(name, a)
        except AssertionError as e:
            bad.append(name)
            print(f"  NOT ON ITS PATH: {e}", flush=True)
        out[name] = a
    if bad:
        sys.exit(f"not written: {sorted(set(bad))}")
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", dest)


if __name__ == "__main__":
    main()
