"""Random Fourier feature map gamma(X) = [sin(2 pi X B), cos(2 pi X B)] (Tancik et al. 2020; Wang, Wang, Perdikaris 2021),
the input encoding the reference's newer hybrid models put in front of their encoder.

In a ``DVPDESolver`` (``args["fourier_features"] = m``) the map runs inside the pre-network kernels: ``forward`` here is the
same formula in torch, for CPU use and for tests.  ``B`` is a buffer, not a parameter: it is saved with the model and never
trained."""
from __future__ import annotations

import math

import torch
import torch.nn as nn


class FourierFeatures(nn.Module):
    """``B`` (in_dim, mapping_size) = randn * scale, drawn at construction; ``forward``: (.., in_dim) -> (.., 2 m), sines
    first, then cosines."""

    def __init__(self, in_dim: int = 3, mapping_size: int = 32, scale: float = 1.0):
        super().__init__()
        if int(in_dim) < 1 or int(mapping_size) < 1:
            raise ValueError(f"FourierFeatures needs in_dim >= 1 and mapping_size >= 1, got {in_dim} and {mapping_size}")
        self.in_dim, self.mapping_size, self.scale = int(in_dim), int(mapping_size), float(scale)
        self.register_buffer("B", torch.randn(self.in_dim, self.mapping_size) * self.scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        turns = x @ self.B.to(x.dtype)
        return torch.cat([torch.sin(2.0 * math.pi * turns), torch.cos(2.0 * math.pi * turns)], dim=-1)
