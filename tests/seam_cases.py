"""Stand-ins for someone else's classes, as tests/test_seam_cpu.py and tests/test_tgs_renderer_cpu.py graft them. They live in a module
of their own, which imports nothing of guassianhand_amd, so that a pickle can name them and a fresh process can load them."""
import torch
import torch.nn as nn


class Plain(nn.Module):
    """One parameter, one buffer and every method a seam overrides, each as a torch statement."""

    def __init__(self, seed=0):
        super().__init__()
        self.fc = nn.Linear(3, 2)
        self.register_buffer("scale", torch.full((2,), 1.0 + seed))

    def forward(self, x, *rest):
        return self.fc(x) * self.scale

    self_attn = forward_gs = forward_single_batch = forward


class Renderer(Plain):
    """A renderer as tgs builds one: configure() counts its calls and takes whatever it is given."""

    def configure(self, *args, **kwargs):
        self.log = getattr(self, "log", []) + [("configure", args, kwargs)]
