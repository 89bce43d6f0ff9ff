"""Record tests/golden/fused_bits.json: run every case of tests/fused_bits_cases.py on the library built from the
checked-out sources and store the digests of W and H.  Run it on the commit whose bits are the reference (the parent
of a change that must not move them):   python tools/record_fused_bits.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fused_bits_cases as fb   # noqa: E402
from pymf_amd import _lib       # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else fb.FIXTURE
    rec, bad = {}, 0
    for cid, name, mode, m, n, k in fb.cases():
        path, hw, hh = fb.run_case(_lib, mode, m, n, k)
        if path != name:
            bad += 1
            print("NOT REACHED: %s ran on %s" % (cid, path), flush=True)
            continue
        rec[cid] = {"kernel": name, "mode": mode, "m": m, "n": n, "k": k, "W": hw, "H": hh}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"niter": fb.NITER, "cases": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases, %d not reached -> %s" % (len(rec), bad, out))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
