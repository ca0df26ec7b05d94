"""dcor._segcall.pack_segments and dcor.dist.shard_segments: the host marshalling every
segment-table entry shares, checked without a device against records written out field by field."""
import ctypes as C

import pytest

# (eps1, eps2, seed, rep_begin, reps): reps = 0 at the front, in the middle and at the end, a
# rep_begin whose range ends at 2^32, seeds above 2^32
PANEL_ROWS = [(1.0, 2.0, 2**33 + 5, 0, 0), (0.5, 0.25, 7, 2**32 - 4, 4), (1.5, 0.5, (5 << 32) + 9, 10, 0),
              (2.0, 2.0, 2**40, 2**32 - 3, 3), (1.0, 1.0, 1, 0, 0)]
PANEL_OUT_ROWS, PANEL_TOTAL = [0, 0, 4, 4, 7], 7
PAIR_COLS = [(0, 1), (3, 0), (2, 2), (1, 3), (0, 2)]
# (eps, seed_ni, seed_int, rep_begin, reps) of the HRS table's rows, the same reps pattern
HRS_ROWS = [(0.25, 2**33 + 1010, 2**34 + 1020, 0, 0), (2.0, 10, 20, 2**32 - 4, 4), (1.05, 2**32, 2**32 + 1, 1001, 0),
            (0.55, 2**63, 2**64 - 1, 2**32 - 3, 3), (2.45, 1, 2, 5, 0)]


def _written(ctype, records):
    """The bytes of a ctype array of max(len, 1) records with every field of `records` assigned."""
    arr = (ctype * max(len(records), 1))()
    for j, fields in enumerate(records):
        for name, value in fields.items():
            setattr(arr[j], name, value)
    return bytes(arr)


def _panel_records():
    return [dict(eps1=e1, eps2=e2, seed=seed, rep_begin=rb, reps=c, out_row=row)
            for (e1, e2, seed, rb, c), row in zip(PANEL_ROWS, PANEL_OUT_ROWS)]


@pytest.mark.parametrize("name", ["SignSegment", "SubgSegment"])
def test_pack_panel_segments(name):
    from dcor import _lib
    from dcor._segcall import pack_segments
    ctype = getattr(_lib, name)
    arr, total = pack_segments(ctype, PANEL_ROWS, 4)
    assert total == PANEL_TOTAL and len(arr) == len(PANEL_ROWS)
    assert bytes(arr) == _written(ctype, _panel_records())


def test_pack_sign_pair_segments():
    from dcor import _lib
    from dcor._segcall import pack_segments
    rows = [(a, b) + r for (a, b), r in zip(PAIR_COLS, PANEL_ROWS)]
    arr, total = pack_segments(_lib.SignPairSegment, rows, 6)
    want = [dict(rec, col_x=a, col_y=b) for (a, b), rec in zip(PAIR_COLS, _panel_records())]
    assert total == PANEL_TOTAL and len(arr) == len(rows)
    assert bytes(arr) == _written(_lib.SignPairSegment, want)


def test_pack_hrs_pair_segments():
    from dcor import _lib
    from dcor._segcall import pack_segments
    rows = [(a, b) + r for (a, b), r in zip(PAIR_COLS, HRS_ROWS)]
    arr, total = pack_segments(_lib.HrsPairSegment, rows, 6)
    want = [dict(eps=e, seed_ni=sn, seed_int=si, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
            for (a, b), (e, sn, si, rb, c), row in zip(PAIR_COLS, HRS_ROWS, PANEL_OUT_ROWS)]
    assert total == PANEL_TOTAL and len(arr) == len(rows)
    assert bytes(arr) == _written(_lib.HrsPairSegment, want)


@pytest.mark.parametrize("name,reps_index", [("SignSegment", 4), ("SubgSegment", 4), ("SignPairSegment", 6),
                                             ("HrsPairSegment", 6)])
def test_pack_no_segments(name, reps_index):
    """No rows: one zeroed record (ctypes has no empty array to pass) and no output rows."""
    from dcor import _lib
    from dcor._segcall import pack_segments
    ctype = getattr(_lib, name)
    arr, total = pack_segments(ctype, [], reps_index)
    assert total == 0 and len(arr) == 1 and bytes(arr) == bytes(C.sizeof(ctype))


def test_pack_takes_numpy_scalars():
    """Rows built from numpy values (a grid of eps, counts from an array) give the same bytes."""
    import numpy as np
    from dcor import _lib
    from dcor._segcall import pack_segments
    rows = [(np.float64(e1), np.float32(e2), np.uint64(seed), np.int64(rb), np.int32(c))
            for e1, e2, seed, rb, c in PANEL_ROWS]
    assert bytes(pack_segments(_lib.SignSegment, rows, 4)[0]) == _written(_lib.SignSegment, _panel_records())


# segment lists per tuple layout (rep_begin index, reps index): zero-length segments at the front,
# in the middle and at the end, totals below and above the worlds, rep_begin near 2^32
SHARD_CASES = [
    (5, 6, [(0, 1, 1.0, 1.0, 2**33 + 1, 0, 0), (0, 2, 2.0, 2.0, 65, 9, 1), (1, 2, 0.2, 0.2, 66, 2**32 - 8, 5),
            (2, 2, 1.0, 1.0, 67, 0, 0), (3, 1, 1.5, 0.7, 68, 1001, 11), (0, 3, 1.0, 1.0, 69, 4, 0)]),
    (5, 6, [(0, 1, 0.25, 10, 20, 3, 0), (1, 0, 2.0, 2**33, 2**34, 7, 2), (2, 3, 1.0, 1, 2, 0, 0)]),   # total 2
    (3, 4, [(1.0, 1.0, 65, 9, 1), (1.0, 1.0, 66, 0, 0), (2.0, 0.5, (5 << 32) + 9, 2**32 - 3, 3)]),      # total 4
    (3, 4, [(1.0, 1.0, 1, 0, 0), (2.0, 2.0, 2, 5, 0)]),                                                # total 0
    (3, 4, []),
]


def _replicates(segs, i_rb, i_reps):
    """Every (key fields, replicate) of segs in order."""
    return [(tuple(v for i, v in enumerate(s) if i not in (i_rb, i_reps)), s[i_rb] + r)
            for s in segs for r in range(s[i_reps])]


@pytest.mark.parametrize("world", [1, 2, 3, 7])
@pytest.mark.parametrize("i_rb,i_reps,segs", SHARD_CASES)
def test_shard_segments_covers_every_replicate_once(world, i_rb, i_reps, segs):
    from dcor.dist import shard, shard_segments
    total = sum(s[i_reps] for s in segs)
    pieces = [shard_segments(segs, i_rb, i_reps, rank, world) for rank in range(world)]
    assert _replicates([p for rank in pieces for p in rank], i_rb, i_reps) == _replicates(segs, i_rb, i_reps)
    for rank in range(world):
        assert sum(p[i_reps] for p in pieces[rank]) == shard(total, rank, world)[1]
        assert all(p[i_reps] > 0 and len(p) == len(segs[0]) for p in pieces[rank])
