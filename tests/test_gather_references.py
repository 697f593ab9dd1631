"""CPU-only: tests/gather_refs.py is sound, and the gather planner of csrc/cache_gather.hip (fgnn_debug_gather_plan: the
function fgnn_gather_rows* plan their launches with) keeps the chunk kernels' 32-bit tile walk inside 2^32 -- every plan
around the window below 2^32 is run through the integer walk simulator.  No launch of that window is ever made on a GPU:
on a library without the rule such a launch never returns."""
import numpy as np
import pytest

import gather_refs as G

TILE4, TILE8 = G.KBLOCK * 4, G.KBLOCK * 8


@pytest.fixture(scope="module")
def lib():
    from fgnn_hip import lib
    lib.load()
    return lib


# ---- the references ------------------------------------------------------------------------------------------------------------

def test_gather_ref_is_the_plain_loop():
    rs = np.random.default_rng(0)
    src = rs.integers(0, 256, size=(16, 5), dtype=np.uint8)
    idx = rs.integers(0, 1 << 20, size=9).astype(np.uint32)
    dst = rs.permutation(12)[:9].astype(np.uint32)
    for use_idx, use_dst, mask, n in [(1, 1, 15, 7), (1, 0, 15, 9), (0, 1, G.NO_MASK, 9), (0, 0, 3, 9), (0, 0, G.NO_MASK, 0)]:
        want = np.full((12, 5), G.POISON, np.uint8)
        for i in range(n):
            want[dst[i] if use_dst else i] = src[((idx[i] if use_idx else i) & mask)]
        got = G.gather_ref(np.full((12, 5), G.POISON, np.uint8), src, n, idx if use_idx else None,
                           dst if use_dst else None, mask)
        assert got.tobytes() == want.tobytes()


def test_split_ref_is_the_stable_partition():
    table, rank = G.cache_table(100, 0.3, seed=1)
    assert (table != G.EMPTY).sum() == 30 and (table[rank[:30]] == np.arange(30)).all()
    nodes = np.random.default_rng(2).integers(0, 100, size=57).astype(np.uint32)
    want = [[], [], [], []]
    for i, v in enumerate(nodes):
        if table[v] == G.EMPTY:
            want[0].append(v), want[1].append(i)
        else:
            want[2].append(table[v]), want[3].append(i)
    for got, w in zip(G.split_ref(table, nodes), want):
        assert got.dtype == np.uint32 and got.tolist() == w
    for frac, miss in ((0.0, 57), (1.0, 0)):
        assert len(G.split_ref(G.cache_table(100, frac, seed=1)[0], nodes)[0]) == miss


# ---- the case table ------------------------------------------------------------------------------------------------------------

def test_case_table_covers_every_axis_value_and_every_path_with_every_count_source():
    for axis, values in G.AXES.items():
        seen = {case_value for case_value in (G.case_row_bytes(c) if axis == "row_bytes" and not c.row_bytes else
                                              getattr(c, axis) for c in G.GATHER_CASES)}
        if axis == "row_bytes":  # "one element" is 1, 2, 4 and 8 bytes
            assert {1, 2, 4, 8} <= seen
            seen = {getattr(c, axis) for c in G.GATHER_CASES}
        assert seen == set(values), (axis, seen)
    pairs = {(G.case_path(c), c.count) for c in G.GATHER_CASES}
    assert pairs >= {(p, k) for p in G.PATHS for k in G.AXES["count"]}
    assert len({G.case_id(c) for c in G.GATHER_CASES}) == len(G.GATHER_CASES)
    for c in G.GATHER_CASES:
        esz = G.DTYPES[c.dtype][1]
        assert G.case_row_bytes(c) % esz == 0 and (not c.align or c.align[1] % esz == 0), c
        assert (c.mask == "pow2") <= (c.form in ("src", "both")) and (c.mask == "noindex") <= (c.form in ("dst", "neither"))
        # a misaligned case keeps whole-chunk rows: only the base pointer sends it to the element kernel
        assert not c.align or G.case_row_bytes(c) % 16 == 0


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_case_shapes_hit_their_targets_and_stay_inside_their_buffers(cus):
    exact = set()
    for c in G.GATHER_CASES:
        elem = G.case_path(c) == "elem"
        unit = G.case_row_bytes(c) // (G.DTYPES[c.dtype][1] if elem else 16)
        tile = G.KBLOCK if elem else G.KBLOCK * G.VEC_UNROLL
        cap = (G.ELEM_WG_PER_CU if elem else G.VEC_WG_PER_CU) * cus
        total = G.case_rows(c, cus) * unit
        if c.rows == "ktiles":
            assert total % tile == 0 and total >= 2 * tile
        if c.rows == "trip2":
            assert total > 2 * cap * tile and total * (G.DTYPES[c.dtype][1] if elem else 16) < 64 << 20
        if c.rows in ("tile-1", "tile", "tile+1") and total == tile + {"tile-1": -1, "tile": 0, "tile+1": 1}[c.rows]:
            exact.add(("elem" if elem else "vec", c.rows))
        if c.rows == "tile+1":
            assert tile < total <= tile + unit
        if c.rows in ("tile-1", "tile"):
            assert max(tile - unit, 0) < total + (c.rows == "tile-1") <= tile or total == unit
        lay = G.build_gather_case(c, cus)
        assert G.layout_stays_inside(lay), G.case_id(c)
        assert lay.want[:G.GUARD_ROWS].min() == G.POISON == lay.want[-G.GUARD_ROWS:].max()
    assert exact >= {("vec", "tile-1"), ("vec", "tile"), ("vec", "tile+1"), ("elem", "tile-1"), ("elem", "tile")}
    # a row wider than one tile is in the table
    assert any(G.case_row_bytes(c) // 16 > G.KBLOCK * G.VEC_UNROLL for c in G.GATHER_CASES if G.case_path(c) != "elem")


# ---- the walk simulator has teeth ----------------------------------------------------------------------------------------------

def test_simulator_accepts_sound_walks_and_names_what_is_wrong_with_the_others():
    assert G.simulate_walk(5, 1, 1024) is None and G.simulate_walk(7 * 1024, 3, 1024) is None
    assert G.simulate_walk(7 * 1024 + 1, 3, 1024) is None and G.simulate_walk(0, 1, 1024) is None
    assert G.simulate_walk((1 << 32) - 1024 * 1024, 1024, 1024) is None  # the rule's last admitted total for that grid
    assert "32-bit" in G.simulate_walk(1 << 32, 1024, 1024)


def test_the_walk_the_parent_admitted_never_ends():
    """(total 0xfffffc00, grid 1024, tile 1024): workgroup 0 is back at tile 0 after 4096 steps; with 1216 workgroups
    (304 CUs) no workgroup ends.  The parent's rule -- total < 0xffffffff -- admits that total."""
    assert G.parent_rule(0xFFFFFC00) and G.parent_rule(0xFFFFFFFE) and not G.parent_rule(0xFFFFFFFF)
    bad = G.simulate_walk(0xFFFFFC00, 1024, 1024)
    assert bad is not None and "workgroup 0 revisits tile 0" in bad
    assert "revisits" in G.simulate_walk(0xFFFFFC00, 1216, 1024)
    assert not G.admissible(0xFFFFFC00, 1024, 1024) and G.admissible((1 << 32) - (1 << 20), 1024, 1024)


# ---- the planner ---------------------------------------------------------------------------------------------------------------

def _totals(grid_cap, tile):
    h = grid_cap * tile
    return [1 << 31, (1 << 32) - h - tile, (1 << 32) - h, (1 << 32) - h + tile, 0xFFFFFC00, 0xFFFFFFFE, 1 << 32,
            (1 << 32) + 5 * tile + 3, (3 << 32) + 17]


@pytest.mark.parametrize("unroll", [4, 8])
@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("cpr", [1, 25, 64, 1024])
def test_every_plan_around_the_window_walks_each_tile_once_and_ends(lib, cpr, cus, unroll):
    tile, grid_cap = G.KBLOCK * unroll, cus * G.VEC_WG_PER_CU
    for target in _totals(grid_cap, tile):
        for rows in sorted({target // cpr, -(-target // cpr)}):
            total = rows * cpr
            plan = lib.debug_gather_plan(rows, 16 * cpr, cus=cus, wg_per_cu=G.VEC_WG_PER_CU, unroll=unroll)
            assert plan is not None, (rows, cpr)
            G.check_plan(plan, rows, cpr, grid_cap, tile)
            one = total < G.SPAN and G.admissible(total, min(-(-total // tile), grid_cap), tile)
            assert (len(plan) == 1) == one, (total, plan[:2])
            # what cannot be sliced is refused exactly where one launch is not admitted
            for kw in (dict(device_sized=True), dict(has_src_index=False, src_row_mask=0xFFFF)):
                got = lib.debug_gather_plan(rows, 16 * cpr, cus=cus, wg_per_cu=G.VEC_WG_PER_CU, unroll=unroll, **kw)
                assert (got == plan) if one else (got is None), (total, kw, got)
            # no mask and no index: slicing moves the base pointers, allowed
            assert lib.debug_gather_plan(rows, 16 * cpr, has_src_index=False, cus=cus, wg_per_cu=G.VEC_WG_PER_CU,
                                         unroll=unroll) == plan


def test_the_planner_slices_what_the_parent_launched_whole(lib):
    plan = lib.debug_gather_plan(0xFFFFFC00, 16, cus=256, wg_per_cu=4, unroll=4)
    assert len(plan) == 2 and plan[0] == (0, 1 << 31, 1024, 1024) and plan[1][:2] == (1 << 31, 0xFFFFFC00 - (1 << 31))
    assert lib.debug_gather_plan(0xFFFFFC00, 16, device_sized=True, cus=256, wg_per_cu=4, unroll=4) is None


def test_planner_small_and_degenerate_requests(lib):
    assert lib.debug_gather_plan(0, 16) == []
    assert lib.debug_gather_plan(1, 16) == [(0, 1, 1, TILE4)]
    assert lib.debug_gather_plan(1, 16400, unroll=8) == [(0, 1, 1, TILE8)]       # 1025 chunks: one ragged tile of 2048
    assert lib.debug_gather_plan(3, 16400) == [(0, 3, 4, TILE4)]
    assert lib.debug_gather_plan(1 << 22, 512, cus=304, wg_per_cu=3) == [(0, 1 << 22, 912, TILE4)]
    L = lib.load()
    assert L.fgnn_debug_gather_plan(10, 12, 0, 1, G.NO_MASK, 256, 4, 4, None, 0) == -1    # not whole chunks
    assert L.fgnn_debug_gather_plan(10, 16, 0, 1, G.NO_MASK, 256, 4, 3, None, 0) == -1    # no such unroll
    assert L.fgnn_debug_gather_plan(10, 16, 0, 1, G.NO_MASK, 0, 4, 4, None, 0) == -1
    assert L.fgnn_debug_gather_plan(10, 16, 0, 1, G.NO_MASK, 256, 4, 4, None, 0) == -2    # no room for the answer
    # a row that the walk cannot cover even alone
    assert lib.debug_gather_plan(1, 16 << 32) is None and lib.debug_gather_plan(1, 16 * ((1 << 32) - 1024)) is None
