"""The lean kernel's blocks (csrc/kta_lean_blocks.h): a workgroup classifies its tiles 64 steps at a time —
one lane per step, two ballots — and its loop walks the masks.  These cases put what the loop and the block rule can get
wrong at a block's edge: the ring crossing it, an exceptional tile, the handover and a change of form at steps 62 to 65,
front flushes off the edges, more and fewer tiles than workgroups, views, and the extrema of tiles that are not taken
or lie past the end.

Every case compares finish() bit for bit with the C oracle (test_gpu_scan_lean._checked) under scan variants 0, 16, 48,
64 and 80, which must agree (test_gpu_scan_plane._five).  With one workgroup a tile's index is its step."""
import numpy as np
import pytest

from test_gpu_scan_lean import LEAN
from test_gpu_scan_packed import BASE_TS, T, _topic
from test_gpu_scan_plane import I32, RAW, _five

pytestmark = pytest.mark.gpu


def _six_byte(cols, tiles):
    """A key of 255 fits no plane: the tile stays a summarised u16 tile, read in the 6-byte form."""
    for t in tiles:
        cols["key_len"][t * T + 9] = 255


def _exceptional(kind, cols, tile, P):
    """Turn one tile into one the lean loop does not take; -> (its header, its mark)."""
    s = tile * T
    if kind == "raw":                                   # a timestamp span of 2^31
        cols["ts_ms"][s + 1], cols["ts_ms"][s + 5] = BASE_TS, BASE_TS + (1 << 31)
        return RAW, 0
    if kind == "i32":                                   # a length that does not fit u16
        cols["val_len"][s + 9] = 70000
        return I32, 0
    assert kind == "part_P"                             # a partition of P: a marked tile whose largest partition does not count
    cols["partition"][s + 7] = P
    return LEAN, 1


# ---- the ring crosses a block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plane", "six_byte"])
@pytest.mark.parametrize("ntiles", [63, 64, 65, 127, 128, 129])
def test_ring_crosses_a_block(ntiles, form):
    for P in (256, 5):
        cols = _topic(ntiles * T, P, seed=71)
        if form == "six_byte":
            _six_byte(cols, range(ntiles))
        _five(P, cols, workgroups=(1,), marks=[int(form == "plane")] * ntiles, expect_hdrs=[LEAN] * ntiles)


# ---- one exceptional tile at a block's edge ----------------------------------------------------------------------------
@pytest.mark.parametrize("step", [62, 63, 64, 65])
@pytest.mark.parametrize("kind", ["raw", "i32", "part_P", "unmarked"])
def test_one_exceptional_tile_at_the_edge(kind, step):
    P, ntiles = 8, 70
    cols = _topic(ntiles * T, P, seed=72)
    hdrs, marks = [LEAN] * ntiles, [1] * ntiles
    if kind == "unmarked":                              # a lean tile among plane tiles: the form changes twice
        _six_byte(cols, [step])
        marks[step] = 0
    else:
        hdrs[step], marks[step] = _exceptional(kind, cols, step, P)
    _five(P, cols, workgroups=(1,), marks=marks, expect_hdrs=hdrs)


# ---- the handover at a block's edge ------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [(3, 17, 30, 44, 63), (3, 17, 30, 44, 64), (3, 17, 30, 44, 65), (60, 61, 62, 63, 64)],
                         ids=["fifth_at_63", "fifth_at_64", "fifth_at_65", "60_to_64"])
@pytest.mark.parametrize("kind", ["raw", "part_P"])
def test_five_exceptional_tiles(kind, steps):
    P, ntiles = 8, 70
    cols = _topic(ntiles * T, P, seed=73)
    hdrs, marks = [LEAN] * ntiles, [1] * ntiles
    for s in steps:
        hdrs[s], marks[s] = _exceptional(kind, cols, s, P)
    _five(P, cols, workgroups=(1,), marks=marks, expect_hdrs=hdrs)


# ---- the two forms around step 64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("six", [range(0, 70, 2), range(1, 70, 2), range(59, 70, 2), range(64, 70), range(0, 64)],
                         ids=["alternate_even", "alternate_odd", "alternate_59_on", "switch_at_64_to_six", "switch_at_64_to_plane"])
def test_forms_around_step_64(six):
    P, ntiles = 8, 70
    cols = _topic(ntiles * T, P, seed=74)
    _six_byte(cols, six)
    _five(P, cols, workgroups=(1,), marks=[int(t not in six) for t in range(ntiles)], expect_hdrs=[LEAN] * ntiles)


# ---- front flushes off the block edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plane", "six_byte"])
def test_front_flushes_off_the_block_edges(form):
    """Others at steps 5 and 40: the 32nd and the 64th taken tile are steps 32 and 65."""
    P, ntiles = 8, 70
    cols = _topic(ntiles * T, P, seed=75)
    hdrs, marks = [LEAN] * ntiles, [int(form == "plane")] * ntiles
    if form == "six_byte":
        _six_byte(cols, range(ntiles))
    hdrs[5], marks[5] = _exceptional("raw", cols, 5, P)
    hdrs[40], marks[40] = _exceptional("i32", cols, 40, P)
    _five(P, cols, workgroups=(1,), marks=marks, expect_hdrs=hdrs)


# ---- more and fewer tiles than a block of every workgroup --------------------------------------------------------------
def test_three_workgroups_over_three_blocks_and_a_tile():
    ntiles = 3 * 64 + 1                                 # workgroup 0 has 65 steps, the others 64
    _five(8, _topic(ntiles * T, 8, seed=76), workgroups=(3,), marks=[1] * ntiles)


def test_eight_workgroups_over_three_tiles():
    _five(8, _topic(3 * T, 8, seed=77), workgroups=(8,), marks=[1] * 3)


def test_a_view_over_66_tiles():
    P, n = 8, 66 * T
    _five(P, _topic(n, P, seed=78), workgroups=(1, 3), marks=[1] * 66, views=((4, n - 4 - 37),))


# ---- extrema of tiles that must not be folded --------------------------------------------------------------------------
def _plain(cols):
    """The topic without its own extremes: no record without a timestamp (it counts as 0, the earliest of all) and no
    message of size 0, so that the records a case plants are the batch's only ones of their kind."""
    t, k, v = cols["ts_ms"], cols["key_len"], cols["val_len"]
    t[t == -1] = BASE_TS + 5
    v[(v >= 0) & (np.maximum(k, 0) + v == 0)] = 1
    return cols


def test_extrema_a_bad_record_with_the_earliest_timestamp():
    """Tile 64 is marked and summarised, but its record of partition P is not counted: neither is its timestamp."""
    P, ntiles = 8, 70
    cols = _plain(_topic(ntiles * T, P, seed=79))
    s = 64 * T + 7
    cols["partition"][s] = P
    cols["ts_ms"][s] = int(cols["ts_ms"].min()) - 1000
    _five(P, cols, workgroups=(1, 3), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles)


def test_extrema_a_cut_off_record_with_the_latest_timestamp():
    P, ntiles = 8, 66
    n = ntiles * T
    cols = _plain(_topic(n, P, seed=80))
    cols["ts_ms"][n - 1] = int(cols["ts_ms"].max()) + 1000
    _five(P, cols, workgroups=(1, 3), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles, views=((0, n - 37),))


@pytest.mark.parametrize("swap", [False, True])
def test_extrema_sizes_of_a_listed_and_a_handed_over_tile(swap):
    """Tiles 64 to 67 are listed and tile 68 is handed over — marked tiles with a record of partition P each.  The bad
    records of tile 64 and of tile 68 are the smallest and the largest message of all, and are not counted."""
    P, ntiles = 8, 70
    cols = _plain(_topic(ntiles * T, P, seed=81))
    for t in range(64, 69):
        cols["partition"][t * T + 7] = P
    small, large = (68, 64) if swap else (64, 68)
    cols["key_len"][small * T + 7], cols["val_len"][small * T + 7] = 0, 0
    cols["key_len"][large * T + 7], cols["val_len"][large * T + 7] = 254, 65534
    sized = cols["val_len"] >= 0
    size = np.maximum(cols["key_len"], 0)[sized] + cols["val_len"][sized]
    assert (size == 0).sum() == 1 and (size == 254 + 65534).sum() == 1   # the two bad records alone
    _five(P, cols, workgroups=(1,), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles)


def test_stale_side_words_past_the_end():
    """130 tiles are uploaded and the first 70 scanned: tiles 70 to 129 hold the earliest timestamps and the extreme
    sizes, and a lane that looks past the end must not fold them."""
    P, ntiles, scanned = 8, 130, 70
    cols = _plain(_topic(ntiles * T, P, seed=82))
    cols["ts_ms"][scanned * T:] -= 10_000_000
    assert cols["ts_ms"][scanned * T:].max() < cols["ts_ms"][:scanned * T].min()
    for t in range(scanned, ntiles):
        cols["key_len"][t * T + 3], cols["val_len"][t * T + 3] = 0, 0
        cols["key_len"][t * T + 4], cols["val_len"][t * T + 4] = 254, 65534
    _five(P, cols, workgroups=(1, 3), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles, views=((0, scanned * T),))
