"""The host side every segment-table entry shares (dcor_sign_panel_launch, dcor_sign_table_launch,
dcor_subg_panel_launch, dcor_hrs_table_launch, dcor_hrs_table_pairwise_launch,
dcor_subg_table_launch): the callers' segment tuples
packed as the entry's C records, and the call itself."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def pack_segments(ctype, rows, reps_index):
    """rows [(col_x, col_y if ctype has them, then ctype's fields up to reps), ...] -> (ctypes array
    of max(len(rows), 1) records, total): out_row is the running sum of the reps before a row, so the
    records lie in segment order, and total their number.  reps_index: where a row holds reps."""
    names = [f for f, _ in ctype._fields_ if f != "out_row"]
    names = [f for f in names if f.startswith("col_")] + [f for f in names if not f.startswith("col_")]
    assert names[reps_index] == "reps"
    kind = dict(ctype._fields_)
    out_row = np.cumsum([0] + [int(r[reps_index]) for r in rows])
    arr = (ctype * max(len(rows), 1))(*[
        ctype(out_row=int(out_row[j]),
              **{f: float(v) if kind[f] is C.c_double else int(v) for f, v in zip(names, r)})
        for j, r in enumerate(rows)])
    return arr, int(out_row[-1])


def run_segment_call(fn, desc, arr, nseg, total, stream=None):
    """fn(desc, arr, nseg, out, stream) on `stream` (the current one by default) -> float64
    [total, 6], copied back: the host waits for the stream, so whatever desc points to only has to
    outlive this call."""
    import torch
    st = torch.cuda.current_stream() if stream is None else stream
    out = torch.empty((max(total, 1), 6), dtype=torch.float64, device="cuda")
    with torch.cuda.stream(st):
        _lib.check(fn(C.byref(desc), arr, nseg, C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        return out[:total].cpu().numpy()
