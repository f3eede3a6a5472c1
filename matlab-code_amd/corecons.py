"""Core consistency (CORCONDIA, Bro & Kiers 2003) of a Tucker core on the host."""
from __future__ import annotations

import numpy as np


def core_consistency(core):
    """100 (1 - sum (core - T)^2 / R) for an R x R x R core, T the superdiagonal array of ones: what
    `Engine.core_consistency` reports for the core `Engine.project` returns on M_n = F_n (F_n'F_n)^+.  Near 100 the CP
    model describes the trilinear part of the data at this R; there is no lower bound.  ValueError unless the core is a
    cube of order 3."""
    G = np.asarray(core, dtype=np.float64)
    if G.ndim != 3 or len(set(G.shape)) != 1 or G.shape[0] < 1:
        raise ValueError('core_consistency: the core must be R x R x R, got shape %r' % (G.shape,))
    R = G.shape[0]
    T = np.zeros_like(G)
    T[np.arange(R), np.arange(R), np.arange(R)] = 1.0
    return float(100.0 * (1.0 - np.sum((G - T) ** 2) / R))
