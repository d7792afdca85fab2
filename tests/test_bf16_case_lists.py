"""CPU checks of the case lists of tests/test_gpu_bf16_exact.py: no GPU involved, but the built library is
(test_grids_reach_every_halo_instantiation loads libsslam_hip.so for its host-side dispatch function, like test_vit_form_api.py
and test_match_pairs_api.py: in a tree that has not been built it raises SslamHipError).

The lists claim to reach every halo instantiation, the 128-cell tail tiles and the refiner's tile counts.  The halo groups come
from the library's own dispatch function (host code; the entry launches by it), not from a restatement of it.
"""
import test_gpu_bf16_exact as E


def test_grids_reach_every_halo_instantiation():
    from sslam_amd import lib
    for (g, f), groups in E.GRIDS.items():
        assert lib.selector_bf16_halo_groups(f, g, 256) == groups, (g, f)
    assert set(E.GRIDS.values()) == {5, 6, 7, 8}
    # the large grids, hidden size 128 and the no-halo knob: the stage form
    assert [lib.selector_bf16_halo_groups(1, g, 256) for g in (128, 160, 192)] == [0, 0, 0]
    assert lib.selector_bf16_halo_groups(3, 28, 128) == 0
    with lib.knobs(SSLAM_CONVBF_NO_HALO=1):
        assert lib.selector_bf16_halo_groups(3, 28, 256) == 0
    assert lib.selector_bf16_halo_groups(3, 28, 256) == 6


def test_grids_reach_the_tail_tiles():
    """SSLAM_CONVBF_TAIL = 2: the cells beyond the last whole round of two 256-cell tiles run as 128-cell tiles."""
    tails = {(g, f): f * g * g - (f * g * g + 255) // 256 // 2 * 2 * 256 for g, f in E.GRIDS}
    assert tails[(24, 2)] == 128 and tails[(16, 5)] == 256 and tails[(40, 1)] == 64 and tails[(60, 1)] == 16


def test_refine_row_counts_reach_the_tile_counts():
    tiles = {}
    for f, k in E.REFINE_ROWS:
        tiles.setdefault((f * k + 63) // 64, set()).add((f * k) % 64 == 0)
    assert set(tiles) == {1, 2, 8, 9, 13, 24, 31} and all(v == {True, False} for v in tiles.values()), tiles
    assert (1, 1) in E.REFINE_ROWS
