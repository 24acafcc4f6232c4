"""Measured-cost scheduling, the host computation (host/irt_sched.cpp sched_order through
irt_debug_sched_order): the block order of every policy and the split work items, against the
rules restated here in numpy, at the smallest sizes where each rule can fail.  No device.
"""
import ctypes as C

import numpy as np
import pytest

import irt

MAX_SPLIT = 4096          # the library's kMaxSplit
GUARD = 0xDEADBEEF        # behind the order buffer: nothing may be written there
EMPTY = 0xFFFFFFFF


def sched_order(cost, num_blocks, tiles_x=1, tile_stride=1, policy=1, split_lg=0, split_factor=1.0,
                num_cu=1, wavewg=True, capacity=None, max_split=MAX_SPLIT):
    """-> (block order, split items, split bitmap, numSplit, the unused tail of the order)."""
    L = irt.lib()
    fn = L.irt_debug_sched_order
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                   C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    cap = num_blocks if capacity is None else capacity
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    assert cost.size == 4 * num_blocks
    mask_words = (4 * cap + 31) // 32
    out = np.full(cap + max_split + mask_words + 8, GUARD, dtype=np.uint32)
    ns = C.c_uint32(12345)
    rc = fn(cost.ctypes.data, num_blocks, tiles_x, tile_stride, policy, split_lg, split_factor, num_cu,
            int(wavewg), cap, max_split, out.ctypes.data, C.byref(ns))
    assert rc == 0, irt.last_error() if hasattr(irt, "last_error") else rc
    assert np.all(out[cap + max_split + mask_words:] == GUARD), "wrote past the order buffer"
    assert np.all(out[num_blocks:cap] == GUARD), "wrote order words past numBlocks"
    return (out[:num_blocks].copy(), out[cap:cap + max_split].copy(),
            out[cap + max_split:cap + max_split + mask_words].copy(), int(ns.value))


def tiles_of(order):
    """The tile sequence of a block order, after checking that each tile's 16 blocks are
    consecutive and ascending and that the order is a permutation."""
    nb = order.size
    assert nb % 16 == 0
    assert np.array_equal(np.sort(order), np.arange(nb, dtype=np.uint32)), "not a permutation"
    rows = order.reshape(-1, 16).astype(np.int64)
    assert np.all(rows[:, 0] % 16 == 0)
    assert np.array_equal(rows, rows[:, :1] + np.arange(16)), "a tile's blocks are not together"
    return (rows[:, 0] // 16).tolist()


def tile_costs(sums, rng):
    """Packet costs (64 per tile) with the given per-tile sums, spread unevenly over the packets."""
    cost = np.zeros((len(sums), 64), dtype=np.uint32)
    for t, s in enumerate(sums):
        cuts = np.sort(rng.integers(0, s + 1, size=63))
        cost[t] = np.diff(np.concatenate(([0], cuts, [s])))
    assert cost.sum(axis=1).tolist() == list(sums)
    return cost.reshape(-1)


@pytest.mark.parametrize("policy", [1, 2, 3])
@pytest.mark.parametrize("nt", [2, 6])
def test_block_order_is_a_permutation_of_whole_tiles(nt, policy):
    rng = np.random.default_rng(100 * nt + policy)
    cost = rng.integers(0, 1000, size=64 * nt).astype(np.uint32)
    order, _, mask, ns = sched_order(cost, 16 * nt, tiles_x=3, tile_stride=1, policy=policy)
    assert sorted(tiles_of(order)) == list(range(nt))
    assert ns == 0 and not mask.any()


def test_policy_1_descending_sums_stable():
    rng = np.random.default_rng(1)
    sums = [5000, 9000, 5000, 9000, 100, 5000]   # ties: equal sums keep index order
    order, _, _, _ = sched_order(tile_costs(sums, rng), 16 * 6, tiles_x=6, policy=1)
    want = np.argsort(-np.asarray(sums), kind="stable").tolist()
    assert want == [1, 3, 0, 2, 5, 4]
    assert tiles_of(order) == want
    # two tiles, the later one costlier; and equal: index order
    assert tiles_of(sched_order(tile_costs([10, 11], rng), 32, policy=1)[0]) == [1, 0]
    assert tiles_of(sched_order(tile_costs([11, 11], rng), 32, policy=1)[0]) == [0, 1]


@pytest.mark.parametrize("tiles_x, stride, band", [(4, 2, 2), (5, 2, 2), (1, 2, 1), (2, 1, 2)])
def test_policy_2_bands_by_sum_tiles_in_index_order(tiles_x, stride, band):
    rng = np.random.default_rng(2)
    sums = [100, 200, 4000, 10, 3000]   # 5 tiles: with a band of 2 the last band is short
    order, _, _, _ = sched_order(tile_costs(sums, rng), 16 * 5, tiles_x=tiles_x, tile_stride=stride, policy=2)
    assert band == max(1, tiles_x // stride)
    bands = [list(range(b, min(5, b + band))) for b in range(0, 5, band)]
    band_sum = np.asarray([sum(sums[t] for t in b) for b in bands])
    want = [t for g in np.argsort(-band_sum, kind="stable") for t in bands[g]]
    if band == 2:
        assert want == [2, 3, 4, 0, 1]   # band sums 300, 4010, 3000
    assert tiles_of(order) == want


def test_policy_2_equal_bands_keep_index_order():
    rng = np.random.default_rng(3)
    order, _, _, _ = sched_order(tile_costs([7, 3, 4, 6, 10], rng), 16 * 5, tiles_x=2, policy=2)
    assert tiles_of(order) == [0, 1, 2, 3, 4]   # sums 10, 10, 10


def test_policy_3_reversed_whatever_the_costs():
    rng = np.random.default_rng(4)
    for sums in ([1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1], [3, 3, 9, 0, 3, 1]):
        order, _, _, _ = sched_order(tile_costs(sums, rng), 16 * 6, tiles_x=3, policy=3)
        assert tiles_of(order) == [5, 4, 3, 2, 1, 0]


def expected_split(cost, split_lg, split_factor, num_cu, max_split=MAX_SPLIT):
    """The rule restated: packets over splitFactor x span, costliest first (ties: lower index),
    at most a tenth of the packets and max_split items; 8 packets per group, a group's parts one
    after the other, each part the group's 8 items."""
    cost = cost.astype(np.int64)
    npk = cost.size
    span = float(cost.sum()) / max(1, 20 * num_cu)
    threshold = float(np.float32(split_factor)) * span
    assert not np.any(np.abs(cost - threshold) <= 0.01 * threshold), "a packet within 1 % of the threshold"
    by_cost = sorted(range(npk), key=lambda k: (-cost[k], k))
    parts = 1 << split_lg
    heavy = []
    for k in by_cost[:npk // 10]:
        if (len(heavy) + 8) * parts > max_split or not cost[k] > threshold:
            break
        heavy.append(k)
    padded = heavy + [None] * (-len(heavy) % 8)
    items = []
    for g in range(0, len(padded), 8):
        for part in range(parts):
            items += [EMPTY if k is None else (k << 8) | (part << 4) | split_lg for k in padded[g:g + 8]]
    mask = np.zeros((npk + 31) // 32, dtype=np.uint32)
    for k in heavy:
        mask[k >> 5] |= np.uint32(1 << (k & 31))
    return heavy, np.asarray(items, dtype=np.uint32), mask


def check_split(cost, nb, split_lg, split_factor, num_cu, max_split=MAX_SPLIT):
    heavy, items, want_mask = expected_split(cost, split_lg, split_factor, num_cu, max_split)
    order, lst, mask, ns = sched_order(cost, nb, tiles_x=2, policy=1, split_lg=split_lg,
                                       split_factor=split_factor, num_cu=num_cu, max_split=max_split)
    tiles_of(order)
    assert ns == items.size and ns % 8 == 0 and ns <= max_split
    assert np.array_equal(lst[:ns], items)
    assert np.all(lst[ns:] == GUARD)
    assert np.array_equal(mask, want_mask)
    # the same facts read off the output alone
    real = lst[:ns][lst[:ns] != EMPTY]
    assert np.all((real & 15) == split_lg)
    assert sorted(set((real >> 8).tolist())) == sorted(heavy)
    for k in heavy:
        at = np.flatnonzero((lst[:ns] >> 8 == k) & (lst[:ns] != EMPTY))
        assert ((lst[at] >> 4) & 15).tolist() == list(range(1 << split_lg))
        assert np.all(np.diff(at) == 8), "the parts of one packet are 8 items apart"
    listed = [int(v) >> 8 for v in lst[:ns] if v != EMPTY and ((int(v) >> 4) & 15) == 0]
    assert listed == heavy, "costliest first"
    return heavy


@pytest.mark.parametrize("split_lg", [1, 2])
def test_split_lists_exactly_the_packets_over_the_threshold(split_lg):
    # 6 tiles = 384 packets of cost 100, 5 heavy ones (two of equal cost): span = total / 20
    cost = np.full(384, 100, dtype=np.uint32)
    for k, v in ((7, 9000), (300, 5000), (64, 7000), (65, 7000), (383, 4000), (200, 1500)):
        cost[k] = v
    # total 71300 -> span 3565: at factor 1 the packets of 4000 and more (1500 is not)
    heavy = check_split(cost, 96, split_lg, 1.0, 1)
    assert heavy == [7, 64, 65, 300, 383]
    # a lower factor (threshold 1247.75) takes the 1500 too
    assert check_split(cost, 96, split_lg, 0.35, 1) == [7, 64, 65, 300, 383, 200]
    # more compute units, a shorter span (3.565): every packet is over it, a tenth is listed
    heavy = check_split(cost, 96, split_lg, 1.0, 1000)
    assert heavy == [7, 64, 65, 300, 383, 200] + list(range(7)) + list(range(8, 33))
    # equal costs: none over the span
    assert check_split(np.full(384, 100, dtype=np.uint32), 96, split_lg, 1.0, 1) == []


@pytest.mark.parametrize("split_lg", [1, 2])
def test_split_at_most_a_tenth_of_the_packets_and_more_than_one_group(split_lg):
    # 2 tiles = 128 packets, 20 of them far over the threshold: only 12 (a tenth) are listed,
    # which is more than one group of 8 (the second group is padded with empty items)
    cost = np.ones(128, dtype=np.uint32)
    idx = np.arange(3, 123, 6)
    cost[idx] = 1000 + 10 * (np.arange(20) % 7)   # with ties
    heavy = check_split(cost, 32, split_lg, 1.0, 4)
    assert len(heavy) == 12
    assert len(set(heavy) & set(idx.tolist())) == 12


def test_split_stops_at_the_item_capacity():
    cost = np.ones(384, dtype=np.uint32)
    cost[::10] = 1000 + np.arange(39)
    heavy = check_split(cost, 96, 2, 1.0, 4, max_split=64)   # (heavy + 8) x 4 parts <= 64
    assert len(heavy) == 9


@pytest.mark.parametrize("split_lg, split_factor, wavewg",
                         [(0, 1.0, True), (2, 0.0, True), (2, -1.0, True), (2, 1.0, False)])
def test_no_splits(split_lg, split_factor, wavewg):
    cost = np.full(384, 100, dtype=np.uint32)
    cost[5] = 100000
    order, lst, mask, ns = sched_order(cost, 96, tiles_x=2, policy=1, split_lg=split_lg,
                                       split_factor=split_factor, num_cu=1, wavewg=wavewg)
    assert ns == 0 and not mask.any() and np.all(lst == GUARD)
    assert tiles_of(order)[0] == 0   # the order is still made


def test_capacity_larger_than_the_grid():
    # the context's buffers keep the capacity of the largest grid seen: list and bitmap sit behind it
    cost = np.full(128, 10, dtype=np.uint32)
    cost[100] = 5000
    order, lst, mask, ns = sched_order(cost, 32, policy=1, split_lg=1, num_cu=1, capacity=80)
    assert tiles_of(order) == [1, 0]
    assert ns == 16 and lst[0] == (100 << 8) | 1 and lst[8] == (100 << 8) | (1 << 4) | 1
    assert mask.size == 10 and mask[3] == 1 << 4 and mask.sum() == 1 << 4
