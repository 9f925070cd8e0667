"""Record tests/golden/conv_bits.json: per case of tests/conv_bits_cases.py, the SHA-256 of every output of the convolution and pooling
entry points (gh_conv3x3_forward / _backward_data, gh_conv2d_forward, gh_maxpool2x2_forward / _backward, gh_maxpool3x3s2_forward) as
the loaded library computes it on the device.

    [GH_RASTER_LIB=/path/to/another/build.so] python tools/record_conv_bits.py --commit REV [--out tests/golden/conv_bits.json]

The fixture is the yardstick of a change that must not move a bit: record it from the library of the commit BEFORE the change
(GH_RASTER_LIB loads a build of that commit; the C-ABI version must match), commit it, then change the kernels;
tests/test_gpu_conv_bits.py recomputes every hash with the tree's own library. Without a ROCm device the tool fails: the bits are
the device's. Where the hashes came from goes into the fixture under "_recorded_from" (the commit the caller names for the
library, the SHA-256 of the library file, the device), a key the tests do not compare."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_bits.json"))
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_conv_bits: no ROCm device; the bits are the device's and nothing is recorded")
    from guassianhand_amd import _lib
    from tests import conv_bits_cases as CB
    _lib.lib()
    dev = torch.device("cuda:0")
    out = {case[0]: CB.hashes(case, dev) for case in CB.CASES}
    with open(_lib.loaded_path(), "rb") as f:
        how = "a build of that commit" + (", loaded through GH_RASTER_LIB" if os.environ.get("GH_RASTER_LIB") else "")
        out["_recorded_from"] = dict(commit=args.commit, what=how, library_sha256=hashlib.sha256(f.read()).hexdigest(),
                                     device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"record_conv_bits: {len(out) - 1} cases from {_lib.loaded_path()} -> {args.out}")


if __name__ == "__main__":
    main()
