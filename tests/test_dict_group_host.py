"""The routing of groupings over dictionary-encoded columns, host side only: which columns a run decodes
(runner.dictionary_columns_to_decode) and when build_frequencies groups on the indices
(grouping.index_path_dictionaries).  No device: the columns are stand-ins with the attributes the rules read."""
from types import SimpleNamespace as NS


def _dictionary(n_entries, dtype="utf8"):
    return NS(n_entries=n_entries, entries=NS(dtype=dtype))


def _chunk(n_rows, **cols):
    return NS(num_rows=n_rows, columns={name: NS(dtype="dict_utf8" if d is not None else "utf8", dictionary=d)
                                        for name, d in cols.items()})


def test_index_path_rule():
    from deequ_amd.grouping import index_path_dictionaries as rule

    d1, d2 = _dictionary(10), _dictionary(5)
    a, b, c = _chunk(8, c=d1, k=None), _chunk(4, c=d1, k=None), _chunk(3, c=d2, k=None)
    assert rule([a], ["c"]) is None  # 10 entries, 8 rows
    assert rule([a, b], ["c"]) == [d1]  # a shared dictionary counts once: 10 <= 12
    assert rule([a, b, c], ["c"]) == [d1, d2]  # 15 <= 15
    assert rule([a, c], ["c"]) is None  # 15 > 11
    assert rule([a, b], ["c", "k"]) is None and rule([a, b], ["k"]) is None and rule([], ["c"]) is None
    assert rule([a, b, _chunk(50, c=None, k=None)], ["c"]) is None  # a plain chunk among them
    assert rule([a, b, _chunk(50, c=_dictionary(1, "large_utf8"), k=None)], ["c"]) is None  # two entry types
    assert rule([a, b], ["missing"]) is None
    assert rule([_chunk(0, c=_dictionary(0))], ["c"]) is not None  # no entries, no rows


def test_single_grouping_column_stays_encoded():
    import deequ_amd as dq
    from deequ_amd.runner import dictionary_columns_to_decode as decode

    schema = [("c", "dict_utf8", True), ("d", "dict_utf8", True), ("k", "i64", True)]
    single = [dq.Uniqueness("c"), dq.Distinctness(["c"]), dq.CountDistinct("c"), dq.UniqueValueRatio("c"),
              dq.Entropy("c"), dq.Histogram("c"), dq.Completeness("c"), dq.ApproxCountDistinct("d"), dq.DataType("d")]
    assert decode(schema, single) == set()
    assert decode(schema, single + [dq.Uniqueness(["c", "k"])]) == {"c"}
    assert decode(schema, single + [dq.MutualInformation("d", "k")]) == {"d"}
    assert decode(schema, single + [dq.PatternMatch("c", r"\d+"), dq.Histogram("d")]) == {"c"}
    assert decode(schema, [dq.Completeness("k", "d = 'x'")]) == {"d"}


def test_decode_counter_exists():
    from deequ_amd.table import Dictionary

    assert Dictionary.decode_calls >= 0 and Dictionary.entries_calls >= 0
