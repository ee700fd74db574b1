#!/usr/bin/env python3
"""Record tests/golden/g19_capi_refusals.json: what a built library answers to every case of tests/_refusal_cases.py -- per case
the return code and the full sml_last_error() text.  Two sections: "host" (the sml_host_* entry points, no GPU) and "gpu" (the
checks only a call with a context reaches; made on an MI355X).  A run rewrites the section it made and keeps the other.

The recording pins the refusals as they were BEFORE the C API was split into capi.hip and capi_ops.hip: it was made with the
library built from the commit before that change and is not regenerated for a later one -- a later library is held to it by
tests/test_capi_refusals_host.py and tests/test_capi_refusals_gpu.py.

usage: python tests/golden/make_golden_refusals.py [--lib <libsml_hip.so of the commit to record>] host|gpu
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "g19_capi_refusals.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("section", choices=("host", "gpu"))
    a = ap.parse_args()
    import _refusal_cases as R
    from sml_amd import _lib
    lib = _lib.load_other(a.lib) if a.lib else _lib.load()
    if a.section == "host":
        got = R.run(lib, R.host_cases())
    else:
        with R.Contexts(lib) as ctx_of:
            got = R.run(lib, R.gpu_cases(), "cuda:0", ctx_of)
    rec = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            rec = json.load(f)
    rec[a.section] = got
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d refused" % (a.section, len(got), sum(1 for rc, _ in got.values() if rc != 0)))


if __name__ == "__main__":
    main()
