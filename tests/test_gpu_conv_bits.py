"""The bits of the two pixel-column convolutions, gh_conv.hip's 3x3 (both directions) and gh_lpips.hip's dense one — two statements of one
MFMA tile that must stay bit-compatible — and of the two pooling kernels, on the device.

Recorded bits: tests/golden/conv_bits.json holds the SHA-256 of every output of every case of tests/conv_bits_cases.py, recorded
(tools/record_conv_bits.py) from the library of the commit its "_recorded_from" names; every hash is recomputed here with the tree's
own library. Agreement: include/gh_lpips.h states its order for Cin > GH_LPIPS_FLAT_CIN as include/gh_conv.h's, so a K = 3, stride 1,
padding 1 gh_conv2d_forward and gh_conv3x3_forward are one fmaf chain per element, a padding tap fmaf(w, 0, acc) in both:
torch.equal, no reference and no tolerance."""
import json
import os

import pytest
import torch

from tests import conv_bits_cases as CB

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bits.json")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from guassianhand_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CB.CASES, ids=CB.IDS)
def test_recorded_bits(dev, golden, case):
    got = CB.hashes(case, dev)
    assert got == golden[case[0]], case[0]


@pytest.mark.parametrize("relu", (False, True), ids=("linear", "relu"))
@pytest.mark.parametrize("bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("shape", CB.AGREE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv2d_k3_is_conv3x3_bitwise(dev, shape, bias, relu):
    from guassianhand_amd import lpips as LP
    from guassianhand_amd import perceptual as P
    N, H, W, Cin, Cout = shape
    x, w, b, _ = (t.to(dev) for t in CB.conv_inputs(N, H, W, Cin, Cout, 3))
    b = b if bias else None
    assert P._conv_applies(x, w, b)                                                         # the HIP path, not a fallback
    runs = []
    with torch.no_grad():
        for chunk in (0, 128):
            runs.append(LP.conv2d(x, w, b, 1, 1, relu, chunk=chunk))
            runs.append(P.conv3x3(x, w, b, relu, chunk=chunk))
    assert runs[0].shape == (N, H, W, Cout) and bool(runs[0].abs().max() > 0)
    for y in runs[1:]:
        assert torch.equal(y, runs[0])
