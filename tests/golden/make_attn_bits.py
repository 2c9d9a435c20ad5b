"""Records tests/golden/attn_bits.npz: what the decode attention entry points compute, bit for bit, on the cases of tests/attn_bits_cases.py
(per case a sha256 of the inputs, the bits of the output and of the K / V rows the call appends).  tests/test_attn_bits_gpu.py holds every
later tree to these bits.

Needs an MI355X and the built tuning library:  python tests/golden/make_attn_bits.py [output.npz]

The fixture is re-recorded only by a change that MEANS to alter the kernels' arithmetic (a rounding fix, another summation order), and that
change says so.  A refactor never re-records: its whole point is that these bits stay.  `source_sha256` names the kernel sources the bits came
from: a sha256 over the sorted names and contents of llamole_amd/csrc/*.hip, llamole_amd/csrc/*.h and include/*.h."""
import glob
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("LLAMOLE_TUNING", "1")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_bits.npz")


def source_digest(root=ROOT):
    files = []
    for pattern in ("llamole_amd/csrc/*.hip", "llamole_amd/csrc/*.h", "include/*.h"):
        files += glob.glob(os.path.join(root, pattern))
    h = hashlib.sha256()
    for f in sorted(files, key=lambda f: os.path.relpath(f, root)):
        h.update(os.path.relpath(f, root).replace(os.sep, "/").encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


if __name__ == "__main__":
    if sys.argv[1:] == ["--digest"]:
        print(source_digest())
        sys.exit(0)
    from llamole_amd import _lib
    from tests import attn_bits_cases as BC
    lib = _lib.load()
    arrays = {"source_sha256": np.array(source_digest())}
    for name in BC.CASES:
        for what, v in BC.run(lib, name).items():
            arrays[f"{name}/{what}"] = np.array(v)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **arrays)
    print("sources", arrays["source_sha256"], "->", out, os.path.getsize(out), "bytes,", len(BC.CASES), "cases")
