"""One device-to-host transfer for many small results, by name.

The pose stage promises ONE read-back per public call.  A Readback keeps that promise without a hand-counted layout: add() records
a device tensor under a name, fetch() concatenates all of them, flattened as float64, into one vector, moves it with one .cpu(), and
hands back {name: array}, each array in the tensor's own shape and the dtype asked for.

float64 carries every value exactly: the integers are counts, indices and statuses bounded by the libraries' size limits (4096
frames, 2^20 edges, int32 at the widest) - far below 2^53, where float64 stops holding every integer - a bool is 0 or 1, and every
float32 value, denormals, infinities and NaN payloads included, is a float64 value."""
from __future__ import annotations

import numpy as np
import torch

_DTYPES = (torch.bool, torch.int32, torch.int64, torch.float32, torch.float64)


class Readback:
    def __init__(self):
        self._pieces = {}                   # name -> (tensor, numpy dtype, rows), in the order added

    def add(self, name: str, tensor: torch.Tensor, dtype, rows: str | None = None) -> None:
        """Record `tensor` (bool, int32, int64, float32 or float64; any shape, empty included) to come back as `dtype`.
        rows: the name of a piece added before, a count the device computed (n_tracks): only that many leading rows of this one
        come back - a buffer sized for the most there could be is cut before it is copied, not after."""
        if name in self._pieces:
            raise ValueError(f"read-back name {name!r} is taken")
        if rows is not None and rows not in self._pieces:
            raise ValueError(f"read-back {name!r}: no piece {rows!r} to count its rows")
        if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _DTYPES:
            raise ValueError(f"read-back {name!r}: a bool, int32, int64, float32 or float64 tensor expected, got {getattr(tensor, 'dtype', type(tensor))}")
        self._pieces[name] = (tensor, np.dtype(dtype), rows)

    def fetch(self) -> dict:
        """{name: array} of everything added (something must have been): one torch.cat, ONE .cpu().  Every array owns its memory."""
        flat = torch.cat([t.detach().reshape(-1).to(torch.float64) for t, _, _ in self._pieces.values()]).cpu().numpy()
        out, at = {}, 0
        for name, (t, dtype, rows) in self._pieces.items():
            piece = flat[at:at + t.numel()].reshape(tuple(t.shape))
            if rows is not None:
                piece = piece[:int(out[rows].reshape(-1)[0])]
            out[name] = piece.astype(dtype)                 # astype copies: the array owns its data
            at += t.numel()
        return out
