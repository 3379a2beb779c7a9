"""Host-side contracts of the optimizer / packing entry points: the tile plan of
the multi-tensor Adam + pack launch (seg_adam_segments_plan), the block and
scratch plan of the batched BatchNorm finish (seg_bn_finish_batch_plan) and the
refusals of seg_pack_filter.  No compute calls: every device pointer is a fake
non-null address that a refused call never touches -- runs without a GPU."""
import ctypes

import pytest

from semanticsegmentation_tensorflow_amd import _lib, ops

OK, EINVAL, EALIGN = 0, 1, 3
TA, TB = 32, 128              # adam_pack_k's tile (csrc/optim.hip)
GROUPS, FOLD_W = 128, 256     # bn_fold_batch_k: row groups, columns per block (csrc/eltwise.hip)
FAKE = 1 << 20


def _ceil(a, b):
    return (a + b - 1) // b


def _adam_table(rows):
    """rows: (rs, a, b, rows_ap, rows_bp, tr_ap); a pad of None = no such copy."""
    arr = (ops.AdamSegment * max(len(rows), 1))()
    off = 0
    for e, (rs, a, b, rap, rbp, tap) in zip(arr, rows):
        e.offset, e.rs, e.a, e.b, e.tile_begin = off, rs, a, b, -7
        if rap is not None:
            e.rows_dst, e.rows_ap, e.rows_bp = FAKE, rap, rbp
        if tap is not None:
            e.tr_dst, e.tr_ap, e.tr_bp = 2 * FAKE, tap, ops.round8(max(b, 1))
        off += (max(rs * a * b, 0) + 3) // 4 * 4
    return arr


def _plan(rows, n=None):
    arr = _adam_table(rows)
    return _lib.load().seg_adam_segments_plan(ctypes.byref(arr), len(rows) if n is None else n), arr


GOOD = [(9, 3, 64, None, None, 8), (9, 72, 136, 72, 136, 72), (16, 2, 64, 8, 64, 8), (1, 1, 64, None, None, None),
        (1, 1, 2, None, None, None), (1, 40, 2, 40, 8, 40), (256, 2, 256, 2, 256, 2), (1, 1, 129, None, None, None),
        (1, 33, 260, 40, 264, None), (1, 32, 128, 32, 128, 32), (49, 31, 127, None, None, 32), (1, 1, 1, 8, 8, 8)]


def test_adam_plan_counts_tiles_and_fills_running_tile_begin():
    total, arr = _plan(GOOD)
    tiles = [rs * _ceil(a, TA) * _ceil(b, TB) for rs, a, b, *_ in GOOD]
    assert total == sum(tiles)
    assert [e.tile_begin for e in arr] == [sum(tiles[:i]) for i in range(len(GOOD))]
    # a prefix of the table is a plan of its own; nothing else of a segment is rewritten
    total3, arr3 = _plan(GOOD, 3)
    assert total3 == sum(tiles[:3]) and arr3[3].tile_begin == -7
    for e, (rs, a, b, rap, rbp, tap) in zip(arr, GOOD):
        assert (e.rs, e.a, e.b) == (rs, a, b)
        assert (e.rows_dst, e.rows_ap, e.rows_bp) == ((FAKE, rap, rbp) if rap is not None else (None, 0, 0))
        assert (e.tr_dst, e.tr_ap) == ((2 * FAKE, tap) if tap is not None else (None, 0))


@pytest.mark.parametrize("bad", [(0, 4, 4, None, None, None), (-1, 4, 4, None, None, None),
                                 (1, 0, 4, None, None, None), (1, -3, 4, None, None, None),
                                 (1, 4, 0, None, None, None), (1, 4, -128, None, None, None),
                                 (1, 9, 8, 8, 8, None),          # rows_ap < a
                                 (1, 8, 9, 8, 8, None),          # rows_bp < b
                                 (1, 9, 8, None, None, 8)],      # tr_ap < a
                         ids=["rs0", "rs-neg", "a0", "a-neg", "b0", "b-neg", "rows_ap", "rows_bp", "tr_ap"])
@pytest.mark.parametrize("where", [0, 1, 2], ids=["first", "middle", "last"])
def test_adam_plan_refuses_a_malformed_segment(bad, where):
    rows = list(GOOD[:2])
    rows.insert(where, bad)
    assert _plan(rows)[0] == -EINVAL
    # the same extents without the copy that was too small are a valid segment
    rs, a, b = bad[:3]
    if min(rs, a, b) > 0:
        rows[where] = (rs, a, b, None, None, None)
        assert _plan(rows)[0] > 0


def test_adam_plan_refuses_an_empty_or_null_table():
    assert _plan(GOOD, 0)[0] == -EINVAL
    assert _plan(GOOD, -1)[0] == -EINVAL
    assert _lib.load().seg_adam_segments_plan(None, 3) == -EINVAL


def test_adam_plan_refuses_more_tiles_than_an_int_holds():
    """The kernel's tile index is an int: a table of more than 2^31 - 1 tiles is
    refused, one of exactly 2^31 - 1 is planned."""
    none = (None, None, None)
    assert _plan([(1 << 20, 1 << 16, 128, *none)])[0] == -EINVAL             # 2^20 * 2^11 = 2^31 tiles
    big = (1 << 20, (1 << 16) - 32, 128, *none)                               # 2^31 - 2^20 tiles
    assert _plan([big])[0] == (1 << 31) - (1 << 20)
    total, arr = _plan([big, ((1 << 20) - 1, 1, 1, *none), (1, 1, 1, *none)], 2)
    assert total == (1 << 31) - 1 and arr[1].tile_begin == (1 << 31) - (1 << 20)
    assert _plan([big, ((1 << 20) - 1, 1, 1, *none), (1, 1, 1, *none)])[0] == -EINVAL
    assert _plan([big, (1 << 20, 1, 1, *none)])[0] == -EINVAL
    assert _plan([GOOD[0], big, (1 << 20, 1, 1, *none)])[0] == -EINVAL


# ---- seg_bn_finish_batch_plan ---------------------------------------------------------------------
BN_TABLE = [(nrows, C, cv) for nrows, C in [(1, 8), (129, 8), (128, 136), (1000, 520), (1, 520), (129, 136),
                                             (1000, 8), (128, 520), (1000, 136), (128, 8), (129, 520), (1, 136)]
            for cv in (C, C - 3, 1)]


def _bn_table(rows):
    arr = (_lib.SegBnFinishSegment * len(rows))()
    for i, (e, (nrows, C, cv)) in enumerate(zip(arr, rows)):
        e.part, e.nrows, e.C, e.cv, e.inv = FAKE, nrows, C, cv, 1.0
        e.dgamma, e.dbeta = 2 * FAKE, 3 * FAKE
        e.scratch, e.a_blk0, e.a_nblk, e.b_blk0, e.b_nblk = 5 * FAKE, -1, -1, -1, -1
    return arr


def _bn_plan(rows, scratch):
    arr = _bn_table(rows)
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    nbytes = _lib.load().seg_bn_finish_batch_plan(ctypes.cast(arr, ctypes.c_void_p), len(rows),
                                                  None if scratch is None else ctypes.c_void_p(scratch),
                                                  ctypes.byref(a), ctypes.byref(b))
    return nbytes, a.value, b.value, arr


@pytest.mark.parametrize("rows", [BN_TABLE, BN_TABLE[::-1], [r for r in BN_TABLE if r[0] <= GROUPS],
                                  [r for r in BN_TABLE if r[0] > GROUPS], BN_TABLE[7:8]],
                         ids=["mixed", "reversed", "none-folded", "all-folded", "single"])
def test_bn_finish_plan_blocks_and_scratch(rows):
    base = 1 << 32
    nbytes, a_blocks, b_blocks, arr = _bn_plan(rows, base)
    folded = [(nrows, C, cv) for nrows, C, cv in rows if nrows > GROUPS]
    assert nbytes == sum(GROUPS * 2 * C * 4 for _, C, _ in folded)
    a = b = 0
    spans = []
    for e, (nrows, C, cv) in zip(arr, rows):
        assert (e.nrows, e.C, e.cv, e.part, e.dgamma, e.dbeta) == (nrows, C, cv, FAKE, 2 * FAKE, 3 * FAKE)
        assert (e.a_blk0, e.b_blk0) == (a, b)
        assert e.b_nblk == _ceil(cv, 8)
        if nrows <= GROUPS:
            assert e.a_nblk == 0 and e.scratch is None
        else:
            assert e.a_nblk == _ceil(2 * C, FOLD_W) * GROUPS
            assert e.scratch is not None and e.scratch % 4 == 0
            spans.append((e.scratch, e.scratch + GROUPS * 2 * C * 4))
        a += e.a_nblk
        b += e.b_nblk
    assert (a_blocks, b_blocks) == (a, b)
    spans.sort()
    for (lo, hi), (lo2, _) in zip(spans, spans[1:] + [(base + nbytes, None)]):
        assert base <= lo and hi <= lo2, "fold scratch slices overlap or leave the buffer"
    # the sizing call (scratch = NULL): the same bytes and grids, no scratch pointers
    nbytes0, a0, b0, arr0 = _bn_plan(rows, None)
    assert (nbytes0, a0, b0) == (nbytes, a_blocks, b_blocks)
    assert all(e.scratch is None for e in arr0)
    assert [(e.a_blk0, e.a_nblk, e.b_blk0, e.b_nblk) for e in arr0] == \
        [(e.a_blk0, e.a_nblk, e.b_blk0, e.b_nblk) for e in arr]


# ---- seg_pack_filter refusals -----------------------------------------------------------------------
def _pack_status(src, R, S, av, bv, ap, bp, mode, dtype=ops.BF16, dst=2 * FAKE):
    return _lib.load().seg_pack_filter(ctypes.c_void_p(src), ctypes.c_void_p(dst), R, S, av, bv, ap, bp, mode,
                                       dtype, None)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pack_filter_refuses_bad_extents(mode):
    assert _pack_status(FAKE, 3, 3, 9, 16, 8, 16, mode) == EINVAL          # a_pad < a_valid
    assert _pack_status(FAKE, 3, 3, 8, 17, 8, 16, mode) == EINVAL          # b_pad < b_valid
    assert _pack_status(FAKE, 3, 3, 8, 12, 8, 12, mode) == EALIGN          # b_pad % 8
    assert _pack_status(FAKE, 3, 3, 8, 2, 8, 4, mode) == EALIGN
    assert _pack_status(FAKE, 3, 3, 3, 16, 3, 16, mode) == EALIGN          # odd a_pad: no mode takes it
    assert _pack_status(FAKE, 3, 3, 1, 16, 1, 16, mode) == EALIGN
    if mode < 2:                                                           # conv copies: a_pad % 8
        for ap in (2, 4, 12):
            assert _pack_status(FAKE, 3, 3, 2, 16, ap, 16, mode) == EALIGN
    assert _lib.load().seg_pack_filter(None, ctypes.c_void_p(FAKE), 3, 3, 8, 16, 8, 16, mode, ops.BF16, None) == EINVAL
    assert _lib.load().seg_pack_filter(ctypes.c_void_p(FAKE), None, 3, 3, 8, 16, 8, 16, mode, ops.BF16, None) == EINVAL


@pytest.mark.parametrize("mode", [4, -1, 17])
def test_pack_filter_refuses_an_unknown_mode(mode):
    assert _pack_status(FAKE, 3, 3, 8, 16, 8, 16, mode) == EINVAL
