"""Row-level random train / test split on the device (the split of ConstraintSuggestionRunner.splitTrainTestSets,
suggestions/ConstraintSuggestionRunner.scala:127-148).

dq_split_rows (include/dqscan.h) draws both selection bitmaps of a chunk in one launch -- a row's side is a pure
function of (seed, global row index), so a table splits the same way however it is chunked -- and the existing stable
compaction (schema.take_rows) builds each side, one index per side per chunk.  Nothing of the selection crosses to the
host but the two counts.  Spark's randomSplit is not restated row for row: its draw depends on the partitioning
("Constraint suggestion").
"""
from __future__ import annotations

import ctypes
import secrets
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

from . import _lib as L
from .schema import _device_args, take_rows
from .table import Table


@dataclass
class SplitBitmaps:
    """The draw of one chunk: the train / test bitmaps (device uint8 tensors of whole 64-bit words plus one) and
    their popcounts."""
    train: object
    test: object
    num_train: int
    num_test: int


@dataclass
class RandomSplit:
    """Both sides (a Table, or one Table per chunk when chunks were given), their row counts and the seed used.
    Unpacks as (train, test)."""
    train: Union[Table, List[Table]]
    test: Union[Table, List[Table]]
    numTrain: int
    numTest: int
    seed: int

    def __iter__(self):
        return iter((self.train, self.test))


def check_ratio(test_ratio: float) -> None:
    if not (0.0 < test_ratio < 1.0):  # ConstraintSuggestionRunner.scala:76
        raise ValueError("requirement failed: Testset ratio must be in ]0, 1[")


def split_bitmaps(n_rows: int, row0: int, seed: int, test_ratio: float, device=None) -> SplitBitmaps:
    """dq_split_rows over rows row0 .. row0 + n_rows - 1."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    words = (n_rows + 63) // 64
    train = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
    test = torch.empty((words + 1) * 8, dtype=torch.uint8, device=dev)
    train[words * 8:].zero_()
    test[words * 8:].zero_()
    d, stream = _device_args(dev)
    nt, ns = ctypes.c_int64(0), ctypes.c_int64(0)
    L.check(L.lib.dq_split_rows(n_rows, row0, seed & ((1 << 64) - 1), test_ratio, train.data_ptr(), test.data_ptr(), d,
                                stream, ctypes.byref(nt), ctypes.byref(ns)))
    return SplitBitmaps(train, test, nt.value, ns.value)


def split_host(n_rows: int, row0: int, seed: int, test_ratio: float):
    """dq_split_rows_host: the same draw on the CPU (no device), a numpy bool array, True = test row."""
    import numpy as np

    out = np.zeros(max(1, n_rows), dtype=np.uint8)
    L.check(L.lib.dq_split_rows_host(n_rows, row0, seed & ((1 << 64) - 1), test_ratio, out.ctypes.data_as(ctypes.c_void_p)))
    return out[:n_rows].astype(bool)


def random_split(data: Union[Table, Sequence[Table]], test_ratio: float, seed: Optional[int] = None) -> RandomSplit:
    """(train, test) of a Table or of a sequence of chunk Tables (then two lists, one Table per chunk, zero-row chunks
    kept).  Chunk k's rows are numbered after the rows of the chunks before it.  seed=None draws one from `secrets`,
    as randomSplit without a seed draws its own; the seed used is on the result."""
    from .table import plain_utf8

    data = plain_utf8(data)  # (dictionary-encoded string columns: read as the plain columns they stand for)
    check_ratio(test_ratio)
    if seed is None:
        seed = secrets.randbits(64)
    single = isinstance(data, Table)
    chunks = [data] if single else list(data)
    if not chunks:
        raise ValueError("random_split: no chunks")
    trains, tests, n_train, n_test, row0 = [], [], 0, 0, 0
    for t in chunks:
        cols = list(t.columns.values())
        b = split_bitmaps(t.num_rows, row0, seed, test_ratio, cols[0].values.device if cols else None)
        trains.append(take_rows(t, b.train, b.num_train))
        tests.append(take_rows(t, b.test, b.num_test))
        n_train += b.num_train
        n_test += b.num_test
        row0 += t.num_rows
    if single:
        return RandomSplit(trains[0], tests[0], n_train, n_test, seed)
    return RandomSplit(trains, tests, n_train, n_test, seed)
