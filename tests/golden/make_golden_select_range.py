#!/usr/bin/env python3
"""The reference's selector over the upper half of the declared NMS range and the smallest grids, produced like
make_golden_wide.py by RUNNING the reference's own KeypointSelector.select_keypoints in the authoring container.

  select_range.npz : 70 tie-free saliency maps (uniform / a band around 0.5 / everything below 0.3) of G in {1, 2, 3, 5, 9, 17, 28},
                     nms_radius 4..8 (every radius at every grid), K in {1, n / 7, n / 2, n}, percentile in {0, 0.1, 0.5, 0.73, 1}

The cases come from tests/select_range_cases.py (golden_case); the fixture stores the maps, the parameters and the reference's
indices and scores: arrays only.  The archive is written with fixed member times, so a second run gives the same bytes.

Usage:  python tests/golden/make_golden_select_range.py
"""
from __future__ import annotations

import io
import os
import zipfile

import numpy as np

import make_golden as mg
import select_range_cases as sc  # (path set up by make_golden)


def save_fixed(name, **arrs):
    """np.savez_compressed with every member stamped 1980-01-01: the bytes depend on the arrays alone."""
    path = os.path.join(mg.HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"wrote {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    M = mg._import_reference()
    sel = mg.load_selector(M["sel"], 0, 256)
    out = {"count": np.int64(sc.GOLDEN_COUNT)}
    params = np.zeros((sc.GOLDEN_COUNT, 3), np.int32)
    pcts = np.zeros(sc.GOLDEN_COUNT, np.float64)
    for s in range(sc.GOLDEN_COUNT):
        m, K, radius, pct = sc.golden_case(s)
        kp, scores, idx = mg.run_select(sel, m, K, radius, pct)      # K <= n: the reference never raises here
        assert idx.shape == (K,) and 0 <= idx.min() and idx.max() < m.size
        params[s], pcts[s] = (m.shape[0], K, radius), pct
        out[f"s{s}_map"] = m
        out[f"s{s}_idx"] = idx.astype(np.int16)
        out[f"s{s}_scores"] = scores.astype(np.float32)
    out["g_k_radius"], out["pct"] = params, pcts
    save_fixed("select_range", **out)


if __name__ == "__main__":
    main()
