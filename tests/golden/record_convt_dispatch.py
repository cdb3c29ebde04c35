"""Record tests/golden/convt_dispatch.json on the MI355X: per case of
tests/test_convt_dispatch_gpu.py the SHA-256 of every output, the launch-hook names in order and
pis_convt2x2_wgrad_ws. Every case runs twice; a case whose two runs differ, or two cases on one shape
that are meant for different arms and wrote the same bits, are reported and the file is not
written. It calls only the C-ABI of the commit before the planner (no pis_debug_convt2x2_algo). Run
from the repo root, at the commit whose kernels are the reference:

    python tests/golden/record_convt_dispatch.py [--lib another/libpis.so] [--out another/file.json]

(--lib: a library built at that commit, run from a later tree; symbols it lacks are not bound)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_convt_dispatch_gpu as t  # noqa: E402
from physics_informed_image_segmentation_amd import _hip  # noqa: E402


def main():
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else t.GOLDEN
    if "--lib" in sys.argv:
        _hip.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
        so = ctypes.CDLL(_hip.LIB_PATH)
        for name in [n for n in _hip.exported_symbols() if not hasattr(so, n)]:
            del _hip._SIGNATURES[name]
    lib = _hip.lib()
    out, bad = {}, []
    for name in t.CASES:
        a, b = t.run_case(lib, name), t.run_case(lib, name)
        print(name, json.dumps(a), flush=True)
        if a != b:
            bad.append(name)
            print(f"  NOT REPEATABLE: second run {json.dumps(b)}", flush=True)
        out[name] = a
    try:
        t.check_discriminates(out)
    except AssertionError as e:
        bad.append(f"same bits from different arms: {e}")
    if bad:
        sys.exit(f"not written: {bad}")
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", dest)


if __name__ == "__main__":
    main()
