#!/usr/bin/env python
"""Generate tests/golden/scene_code_fixture.npz by running the REFERENCE's TriplaneLearnablePositionalEmbedding.detokenize
(tgs/models/tokenizers/triplane_texture.py:45-57) and TriplaneUpsampleNetwork (tgs/models/networks_texture.py:30-54) on the CPU, with
the three statements around them (infer_one_shot.py:266, 270, 271) written out.

Runs only where the reference tree is present; the resulting .npz is data (inputs, weights and recorded outputs) and is committed;
nothing of the reference travels. The reference modules are imported under the stub modules of make_host_fixtures.py and built the
reference's way (`__new__`, a stand-in cfg, configure()). Two cases (B, Ci, Co, Np, S):

    a   (1, 512, 80, 2, 4)        the config's channels on a small plane
    b   (2, 33, 7, 2, 3)          odd everything, two batch elements

each with a (Co, 2S, 4S) plane bias of which the statements read the first 2S columns, as `map_bias` (80, 64, 128) is read through
its first 64. Everything lies on exact grids, stored as int8 (`*_q`, value = q * scale): tokens are multiples of 1/16 within +-2.5,
weights non-zero multiples of 1/256 within +-24/256, both biases multiples of 1/256, cotangents multiples of 1/8. Every product is
then a multiple of 2^-12 and a 512-term sum stays below 2^7, so every sum of the forward and of the three gradients is exact in
float32 in any order: the recorded values hold bit for bit on any host and any device. Per case <t>:

    <t>_dims                      B, Ci, Co, Np, S
    <t>_tok_a_q, <t>_tok_b_q      the two token tensors (B, Ci, Np S^2)
    <t>_weight_q, <t>_bias_q      upsample.weight (Ci, Co, 2, 2), upsample.bias (Co,)
    <t>_plane_bias_q              (Co, 2S, 4S)
    <t>_cot_q                     the cotangent of `out`
    <t>_out                       (B, 1, Co, 2S, Np 2S)
    <t>_d_tokens                  the gradient of sum(out * cot) in tokens_texture (and, equally, in tokens_shade)
    <t>_d_plane_bias              its gradient in the plane bias, (Co, 2S, 4S)
    init_keys, init_shapes        the state dict configure() leaves: names, and shapes padded to four entries

Usage: python tests/golden/make_scene_code_fixture.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_host_fixtures as host  # noqa: E402  (applies tests/cpu_numerics.py on one thread before torch is imported)
import torch  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scene_code_fixture.npz")
X_SCALE, W_SCALE, C_SCALE = 1.0 / 16, 1.0 / 256, 1.0 / 8
CASES = {"a": (1, 512, 80, 2, 4), "b": (2, 33, 7, 2, 3)}


def build(cls, **cfg):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.cfg = types.SimpleNamespace(**cfg)
    m.configure()
    return m


def main():
    host.install_stubs([])
    sys.path.insert(0, REF)
    from tgs.models.networks_texture import TriplaneUpsampleNetwork
    from tgs.models.tokenizers.triplane_texture import TriplaneLearnablePositionalEmbedding

    g = torch.Generator().manual_seed(47)
    out = {"scales": np.array([X_SCALE, W_SCALE, C_SCALE])}
    for t, (B, Ci, Co, Np, S) in CASES.items():
        tokenizer = build(TriplaneLearnablePositionalEmbedding, plane_size=S, num_channels=Ci, n_plane=Np)
        post = build(TriplaneUpsampleNetwork, in_channels=Ci, out_channels=Co, n_plane=Np)
        if t == "a":
            sd = post.state_dict()
            out["init_keys"] = np.array(list(sd.keys()))
            out["init_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()])
        T = Np * S * S
        aq = torch.randint(-40, 41, (B, Ci, T), generator=g, dtype=torch.int8)
        bq = torch.randint(-40, 41, (B, Ci, T), generator=g, dtype=torch.int8)
        keep = (aq.int() + bq.int()).abs() <= 40                       # the sum stays within +-2.5
        bq = torch.where(keep, bq, -bq)
        assert int((aq.int() + bq.int()).abs().max()) <= 40
        wq = torch.randint(-24, 25, (Ci, Co, 2, 2), generator=g, dtype=torch.int8)
        wq[wq == 0] = 1                                               # non-zero weights
        cbq = torch.randint(-100, 101, (Co,), generator=g, dtype=torch.int8)
        pbq = torch.randint(-100, 101, (Co, 2 * S, 4 * S), generator=g, dtype=torch.int8)
        cq = torch.randint(-24, 25, (B, 1, Co, 2 * S, Np * 2 * S), generator=g, dtype=torch.int8)
        with torch.no_grad():
            post.upsample.weight.copy_(wq.float() * W_SCALE)
            post.upsample.bias.copy_(cbq.float() * W_SCALE)
        tokens_texture = (aq.float() * X_SCALE).requires_grad_(True)
        tokens_shade = (bq.float() * X_SCALE).requires_grad_(True)
        map_bias = (pbq.float() * W_SCALE).requires_grad_(True)
        w = 2 * S                                                     # the statements' literal 64 at S = 32

        tokens = tokens_texture + tokens_shade
        scene_codes_texture = tokenizer.detokenize(tokens)
        scene_codes_texture = post(scene_codes_texture)
        scene_codes_texture = torch.cat([scene_codes_texture[:, 0], scene_codes_texture[:, 1]], dim=-1).unsqueeze(1)
        scene_codes_texture = scene_codes_texture + torch.cat([map_bias[..., :w], map_bias[..., :w]], dim=-1)

        (scene_codes_texture * (cq.float() * C_SCALE)).sum().backward()
        assert torch.equal(tokens_texture.grad, tokens_shade.grad)
        assert float(map_bias.grad[..., w:].abs().max()) == 0.0
        out[f"{t}_dims"] = np.array([B, Ci, Co, Np, S])
        out[f"{t}_tok_a_q"], out[f"{t}_tok_b_q"] = aq.numpy(), bq.numpy()
        out[f"{t}_weight_q"], out[f"{t}_bias_q"], out[f"{t}_plane_bias_q"], out[f"{t}_cot_q"] = wq.numpy(), cbq.numpy(), pbq.numpy(), cq.numpy()
        out[f"{t}_out"] = scene_codes_texture.detach().numpy()
        out[f"{t}_d_tokens"] = tokens_texture.grad.numpy()
        out[f"{t}_d_plane_bias"] = map_bias.grad.numpy()

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 300_000, size
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
