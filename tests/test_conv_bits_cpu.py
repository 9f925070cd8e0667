"""tests/golden/conv_bits.json and tests/conv_bits_cases.py without a GPU: the fixture holds exactly the cases of the list — none is
missing, none is skipped, none is left over — and the input builder still produces the values the fixture was recorded on."""
import json
import math
import os

import torch

from tests import conv_bits_cases as CB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bits.json")
OUTPUTS = {"conv3x3": {"y", "dx"}, "conv2d": {"y"}, "pool2x2": {"y", "choice", "dx"}, "pool3x3s2": {"y"}}


def test_fixture_holds_exactly_the_cases():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(set(CB.IDS)) == len(CB.IDS) == 5 * 2 * 4 + 7 * 2 * 4 + 4 + 4 * 3
    assert set(golden["_recorded_from"]) == {"commit", "what", "library_sha256", "device"}     # where the hashes came from: not compared
    assert set(golden) - {"_recorded_from"} == set(CB.IDS)
    for name, kind, prm in CB.CASES:
        want = OUTPUTS[kind] | ({"gate"} if kind == "conv3x3" and prm[5] else set())
        assert set(golden[name]) == want, name
        assert all(len(h) == 64 and int(h, 16) >= 0 for h in golden[name].values()), name


def test_input_builder_reproduces_literal_values():
    """(flat index, salt, scale) -> the float32 value, worked out with Python's integers and correctly rounded doubles."""
    lit = ((0, 1, 1.0, "-0x1.fffcp-2"), (1, 1, 1.0, "0x1.fbe9c2p-3"), (65520, 7, 1.0, "-0x1.fba9bep-3"), (1000003, 12345, 1.0, "0x1.037334p-3"),
           (5, 2, 2.0 / math.sqrt(27), "0x1.7a55dp-4"), (123456, 99, 2.0 / math.sqrt(25 * 64), "0x1.a29554p-7"))
    for i, salt, scale, want in lit:
        got = CB.unit((i + 1,), salt, scale)
        assert got.dtype == torch.float32 and float(got[i]) == float.fromhex(want), (i, salt, got[i].item().hex())
    assert CB.small_ints((12,), 9).tolist() == [2, 1, -1, 2, 1, -1, 2, 0, -1, 2, 0, -2]
    x, w, b, g = CB.conv_inputs(1, 2, 3, 17, 6, 3)
    assert (x.shape, w.shape, b.shape, g.shape) == ((1, 2, 3, 17), (6, 17, 3, 3), (6,), (1, 2, 3, 6))
    assert float(w.abs().max()) <= 1.0 / math.sqrt(9 * 17) and float(x.abs().max()) <= 1.0


def test_pool_inputs_have_ties_infinities_and_nans():
    x, g = CB.pool2x2_input(7, 8)
    assert g.shape == (2, 3, 4, 3) and int(torch.isnan(x).sum()) == 4
    assert bool((x[1, :2, :2, 1] == float("-inf")).all()) and float(x[1, 1, 2, 2]) == -2.0 and float(x[1, 0, 2, 2]) == float("-inf")
    win = x[0, 2:4, 2:4, 0].reshape(-1)
    assert int((win == win.max()).sum()) >= 2                                              # a tie for the maximum
    x = CB.pool3x3_input(4, 9, 7)
    assert bool((x[1, :3, :3] == float("-inf")).all()) and bool(torch.isnan(x[2, 1, 1]).all()) and bool(torch.isnan(x[2, 3, 8]).all())
    assert x[1, 3].unique().numel() <= 3
