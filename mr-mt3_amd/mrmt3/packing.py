"""Host side of packed decoder training (csrc/pack.hip): row lengths, the capacity granule and Tcap.

A target row is padded to L with -100 and the loss ignores those positions (tasks/mt3_net.py:32-35).  Under the causal decoder
nothing after a row's last scored label reaches a scored position, so the decoder only needs each row's prefix of
len_b = 1 + (last t with labels[b, t] != -100) tokens (0 for a row with none).  The prefixes are laid end to end, T = sum len_b
rows, padded to the capacity Tcap = T rounded up to the granule G = max(256, roundup(B*L/16, 256)): at most 16 capacities (and
so 16 captured graphs) per batch shape.  Tcap = B*L means nothing is saved: the caller takes the dense path.
"""
from __future__ import annotations

import numpy as np


def row_lengths(labels) -> np.ndarray:
    """len_b of a [B, L] integer array (numpy or a CPU tensor): 1 + the last position whose label is not -100, else 0."""
    lab = np.asarray(labels)
    B, L = lab.shape
    scored = lab != -100
    last = L - np.argmax(scored[:, ::-1], axis=1)
    return np.where(scored.any(axis=1), last, 0).astype(np.int32)


def granule(B: int, L: int) -> int:
    return max(256, -(-(B * L) // (16 * 256)) * 256)


def capacity(lengths, B: int, L: int) -> int:
    """Tcap for these row lengths: T rounded up to the granule (at least one granule), at most B*L (= the dense path)."""
    G = granule(B, L)
    T = int(np.sum(lengths))
    return min(max(G, -(-T // G) * G), B * L)
