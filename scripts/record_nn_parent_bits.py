#!/usr/bin/env python3
"""Record tests/golden/nn_parent_bits.json: the digests tests/test_nn_parent_bits.py compares against.

    python scripts/record_nn_parent_bits.py [TREE] > tests/golden/nn_parent_bits.json

Runs the test module's own cases (its cases() makes the seeded inputs) on device 0 with the library of TREE -- a checkout, with its library built,
of the commit whose bits are to be pinned: the one before the U-Net moved onto nn_convk, which has RunConv3x3 and RunConv like this one.  Without
TREE: this tree, which is only good for seeing that nothing moved."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, TREE)       # tracerboy_amd comes from here


def main():
    import test_nn_parent_bits as cases
    from tracerboy_amd import api, build
    assert os.path.dirname(os.path.dirname(os.path.abspath(api.__file__))) == TREE
    digests = {}
    with tempfile.TemporaryDirectory() as tmp, api.TracerBoy(0) as tb:
        for name, run in cases.cases():
            digests[name] = cases.digest(run(tb, tmp))
    print(json.dumps({"what": "SHA-256 of dtype, shape and bytes of every case of tests/test_nn_parent_bits.py, recorded on an MI355X with the library of "
                              "the commit before nn_conv3x3 was retired", "kernel_digest": build.kernel_digest(), "digests": digests}, indent=1))


if __name__ == "__main__":
    main()
