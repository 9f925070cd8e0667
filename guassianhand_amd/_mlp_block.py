"""The reference's MLP_block (tgs/models/verts_refinement.py:16-32) and what its two users here — vert_mlp.py (vert_valid,
vert_pos_refinement) and cond.py (additional_features_fc) — do with it: its parameters in the order of GhVertParams / GhCondParams,
the reference's initialisation, and whether its dropout is live."""
from __future__ import annotations

import torch.nn as nn
import torch.nn.functional as F


class _MLPBlock(nn.Module):
    """The reference's MLP_block: the sub-module names are its state-dict keys."""

    def __init__(self, in_dim: int, hid_dim: int, dropout: float = 0.1):
        super().__init__()
        self.layer_norm = nn.LayerNorm(in_dim, eps=1e-6)
        self.fc1 = nn.Linear(in_dim, hid_dim)
        self.fc2 = nn.Linear(hid_dim, hid_dim)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, x):
        return self.dropout2(self.fc2(self.dropout1(F.relu(self.fc1(self.layer_norm(x))))))


def block_params(ff):
    """The six tensors of an MLP_block (the reference's or _MLPBlock) in GhVertParams / GhCondParams order."""
    return [ff.layer_norm.weight, ff.layer_norm.bias, ff.fc1.weight, ff.fc1.bias, ff.fc2.weight, ff.fc2.bias]


def init_linears(module: nn.Module) -> None:
    """weights_init (verts_refinement.py:5-13) over the module's nn.Linear layers: Xavier-uniform weights, zero biases."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0.0)


def dropout_live(module: nn.Module, ff) -> bool:
    """The module is in train mode and either dropout of its MLP_block `ff` has p > 0: the kernels, which have no dropout, stand aside."""
    return bool(module.training) and any(float(getattr(d, "p", 0.0)) > 0 for d in (ff.dropout1, ff.dropout2))
