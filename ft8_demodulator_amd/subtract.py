"""Subtract-and-redecode with more than two passes (ft8_set_subtract): the host-side checks and the
NumPy restatement of the merge an FT8_FLAG_SUBTRACT batch applies after every pass from the second on
(csrc/subtract.hip k_merge; include/ft8hip.h states the n-pass batch).

Nothing here decodes: the restatement rearranges records the device produced, so that a test (or a
caller) can rebuild a batch's output from the library's own stage calls, byte for byte.
"""
from __future__ import annotations

import numpy as np

MIN_PASSES, MAX_PASSES = 2, 4   # FT8_SUBTRACT_MAX_PASSES
DEFAULT_PASSES = 2


def check_passes(n) -> int:
    """The pass count of an FT8_FLAG_SUBTRACT batch as ft8_set_subtract takes it: an integer in
    [2, 4] -> int; ValueError for anything the library refuses (bool and float included)."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"subtract takes a pass count in [{MIN_PASSES}, {MAX_PASSES}], got {n!r}")
    if not MIN_PASSES <= int(n) <= MAX_PASSES:
        raise ValueError(f"subtract takes a pass count in [{MIN_PASSES}, {MAX_PASSES}], got {n!r}")
    return int(n)


def passes_of(subtract):
    """SlotDecoder's / decode_ft8_message's `subtract` argument -> the pass count, or None for off:
    None / False: off, True: 2 passes, else check_passes."""
    if subtract is None or subtract is False:
        return None
    if subtract is True:
        return DEFAULT_PASSES
    return check_passes(subtract)


def merge_restate(acc: np.ndarray, recs: np.ndarray) -> np.ndarray:
    """One slot's accumulated records after a further pass: `acc` as it is, then the ok rows of `recs`
    (that pass's records) whose payload no row of `acc` carries -- only the rows present before the
    pass count as seen, so two new rows of one payload are both appended -- in `recs` order, with bit 0
    of pass_index set and every other bit kept (the coherent bits 1 to 3, the a-priori hypothesis in
    the high nibble).  acc, recs: structured ft8_result arrays (_lib.RESULT_DTYPE) -> one such array."""
    seen = {bytes(r["payload"]) for r in acc}
    new = np.array([j for j, r in enumerate(recs) if r["ok"] and bytes(r["payload"]) not in seen], dtype=np.int64)
    tail = recs[new].copy()
    tail["pass_index"] |= 1
    return np.concatenate([acc, tail])


def subtract_index(record) -> int:
    """Bit 0 of a record's pass_index: 1 when a pass >= 2 appended it (decoded from a residual)."""
    return int(record["pass_index"]) & 1


def pass_of(counts_row, i) -> int:
    """The 1-based pass that appended row i of a slot, from the slot's row of ft8_subtract_counts
    (the uncapped count after each pass, non-decreasing): the first pass whose count exceeds i.
    IndexError when the slot has no row i."""
    i = int(i)
    if i < 0:
        raise IndexError(f"row {i}")
    for k, c in enumerate(counts_row):
        if i < int(c):
            return k + 1
    raise IndexError(f"row {i} is past the slot's {int(counts_row[-1]) if len(counts_row) else 0} rows")
