"""Plain-Python restatement of the train / test draw of dq_split_rows (include/dqscan.h): row g is a test row iff
(XXH64(8 little-endian bytes of g, seed) >> 11) * 2^-53 < test_ratio.  The hash comes from the xxhash module when it
is installed, else from the 8-byte case of XXH64 written out below; both are independent of deequ_amd/csrc."""
from __future__ import annotations

import struct

M = (1 << 64) - 1
P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                      0x27D4EB2F165667C5)


def _rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (64 - r))) & M


def xxh64_of_8_bytes(data: bytes, seed: int) -> int:
    """XXH64 of exactly 8 bytes: no 32-byte stripe, one 8-byte round, the avalanche."""
    assert len(data) == 8
    (lane,) = struct.unpack("<Q", data)
    h = (seed + P5 + 8) & M
    k = (_rotl((lane * P2) & M, 31) * P1) & M
    h = (_rotl(h ^ k, 27) * P1 + P4) & M
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    return h ^ (h >> 32)


try:
    import xxhash

    def hash_row(g: int, seed: int) -> int:
        return xxhash.xxh64_intdigest(struct.pack("<Q", g), seed & M)
except ImportError:  # pragma: no cover
    def hash_row(g: int, seed: int) -> int:
        return xxh64_of_8_bytes(struct.pack("<Q", g), seed & M)


def is_test(g: int, seed: int, test_ratio: float) -> bool:
    return (hash_row(g, seed) >> 11) * 2.0 ** -53 < test_ratio


def split(n_rows: int, row0: int, seed: int, test_ratio: float):
    """[True for a test row, False for a training row] of rows row0 .. row0 + n_rows - 1."""
    return [is_test(row0 + r, seed, test_ratio) for r in range(n_rows)]
