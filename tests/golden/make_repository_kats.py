"""Write repository_kats.json: what the reference's repository tests pin, as data.

Paths are relative to src/test/scala/com/amazon/deequ/repository/.  Transcribed by hand:
  * AnalysisResultTest.scala: the analysis of :326-332 over dfFull (utils/FixtureSupport.scala:64-73), whose four
    metric values its expected rows state, and every expected rows / JSON pair of :39-313;
  * AnalysisResultSerdeTest.scala: the analyzer / metric pairs of the round-trip tests (:35-82, :102-103, :148-149,
    :158-164) and SimpleResultSerdeTest's analysis and expected string (:197-234).
The reference pins no serialized AnalysisResult text (its serde tests only round-trip), so `serde_layout` is written
here from the field names of the serializers in src/main/scala/.../repository/AnalysisResultSerde.scala:108-594: it pins
this project's reading of that layout, not a file the reference wrote.
"""
import json
import os

DATE_ONE = 1507975810  # LocalDate.of(2017, 10, 14).atTime(10, 10, 10).toEpochSecond(ZoneOffset.UTC)


def dm(entity, name, instance, value):
    return {"metricName": "DoubleMetric", "entity": entity, "instance": instance, "name": name, "value": value}


def hist(column, bins, values):
    return {"metricName": "HistogramMetric", "column": column, "numberOfBins": bins,
            "value": {"numberOfBins": bins, "values": {k: {"absolute": a, "ratio": r} for k, (a, r) in values.items()}}}


FIVE = dm("Column", "Completeness", "ColumnA", 5.0)

# AnalysisResultSerdeTest.scala:35-82; a later duplicate key of the Scala Map (Correlation, :51) replaces the earlier one
serde_metric_map = [
    [{"analyzerName": "Size"}, dm("Column", "Size", "*", 5.0)],
    [{"analyzerName": "Completeness", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "Compliance", "instance": "rule1", "predicate": "att1 > 3"}, FIVE],
    [{"analyzerName": "ApproxCountDistinct", "column": "columnA", "where": "test"}, FIVE],
    [{"analyzerName": "CountDistinct", "columns": ["columnA", "columnB"]}, FIVE],
    [{"analyzerName": "Distinctness", "columns": ["columnA", "columnB"]}, FIVE],
    [{"analyzerName": "Correlation", "firstColumn": "firstColumn", "secondColumn": "secondColumn", "where": "test"}, FIVE],
    [{"analyzerName": "UniqueValueRatio", "columns": ["columnA", "columnB"]}, FIVE],
    [{"analyzerName": "Uniqueness", "columns": ["ColumnA"]}, FIVE],
    [{"analyzerName": "Uniqueness", "columns": ["ColumnA", "ColumnB"]}, FIVE],
    # Histogram("ColumnA") and Histogram("ColumnA", None) are one key (:57-62): the second metric stays
    [{"analyzerName": "Histogram", "column": "ColumnA", "maxDetailBins": 1000},
     hist("ColumnA", 10, {"some": (10, 0.5), "other": (0, 0.0)})],
    [{"analyzerName": "Histogram", "column": "ColumnA", "maxDetailBins": 5}, hist("ColumnA", 10, {"some": (10, 0.5)})],
    [{"analyzerName": "Entropy", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "MutualInformation", "columns": ["ColumnA", "ColumnB"]}, FIVE],
    [{"analyzerName": "Minimum", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "Maximum", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "Mean", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "Sum", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "StandardDeviation", "column": "ColumnA"}, FIVE],
    [{"analyzerName": "DataType", "column": "ColumnA"}, FIVE],
]


def result(date, tags, metric_map):
    return {"resultKey": {"dataSetDate": date, "tags": tags},
            "analyzerContext": {"metricMap": [{"analyzer": a, "metric": m} for a, m in metric_map]}}


serde_layout = {
    "source": "AnalysisResultSerdeTest.scala:35-93, :148-149, :158-164; layout of AnalysisResultSerde.scala:108-594",
    "results": [
        result(DATE_ONE, {"Region": "EU"}, serde_metric_map),
        result(DATE_ONE, {"Region": "NA"}, serde_metric_map),
        result(0, {}, [[{"analyzerName": "ApproxQuantile", "column": "col", "quantile": 0.5, "relativeError": 0.2},
                        dm("Column", "ApproxQuantile", "col", 0.5)]]),
        result(0, {}, [[{"analyzerName": "ApproxQuantiles", "column": "col", "quantiles": "0.25,0.5,0.75",
                         "relativeError": 0.2},
                        {"metricName": "KeyedDoubleMetric", "entity": "Column", "instance": "col",
                         "name": "ApproxQuantiles", "value": {"0.25": 10.0, "0.5": 20.0, "0.75": 30.0}}]]),
    ],
}

# AnalysisResultTest.scala:326-332 over dfFull, values from the expected rows of :50-55
context_dfFull = [
    [{"analyzerName": "Size"}, dm("Dataset", "Size", "*", 4.0)],
    [{"analyzerName": "Distinctness", "columns": ["item"]}, dm("Column", "Distinctness", "item", 1.0)],
    [{"analyzerName": "Completeness", "column": "att1"}, dm("Column", "Completeness", "att1", 1.0)],
    [{"analyzerName": "Uniqueness", "columns": ["att1", "att2"]}, dm("Mutlicolumn", "Uniqueness", "att1,att2", 0.25)],
]

ROWS = [("Dataset", "*", "Size", 4.0), ("Column", "item", "Distinctness", 1.0),
        ("Column", "att1", "Completeness", 1.0), ("Mutlicolumn", "att1,att2", "Uniqueness", 0.25)]


def rows(which, tag_column):
    return [{"entity": e, "instance": i, "name": n, "value": v, "dataset_date": DATE_ONE, tag_column: "EU"}
            for e, i, n, v in ROWS if n in which]


def expected_json(which, tag_column):  # the string of e.g. :70-80, $DATE_ONE substituted, in the test's row order
    order = ["Size", "Completeness", "Distinctness", "Uniqueness"]
    by_name = {n: (e, i, n, v) for e, i, n, v in ROWS}
    parts = []
    for name in order:
        if name not in which:
            continue
        e, i, n, v = by_name[name]
        parts.append(f'{{"entity":"{e}","instance":"{i}","name":"{n}","value":{v},'
                     f'"{tag_column}":"EU", "dataset_date":{DATE_ONE}}}')
    return "[" + ",".join(parts) + "]"


ALL = ["Size", "Distinctness", "Completeness", "Uniqueness"]
REQUESTED = [{"analyzerName": "Completeness", "column": "att1"}, {"analyzerName": "Uniqueness", "columns": ["att1", "att2"]}]
analysis_result_cases = [
    {"name": "formatted as expected", "source": "AnalysisResultTest.scala:39-84", "tags": {"Region": "EU"},
     "forAnalyzers": [], "withTags": [], "rows": rows(ALL, "region"), "json": expected_json(ALL, "region")},
    {"name": "only requested metrics", "source": "AnalysisResultTest.scala:86-132", "tags": {"Region": "EU"},
     "forAnalyzers": REQUESTED, "withTags": [], "rows": rows(["Completeness", "Uniqueness"], "region"),
     "json": expected_json(["Completeness", "Uniqueness"], "region")},
    {"name": "tag names into valid column names", "source": "AnalysisResultTest.scala:134-179",
     "tags": {"Re%%^gion!/": "EU"}, "forAnalyzers": [], "withTags": [], "rows": rows(ALL, "region"),
     "json": expected_json(ALL, "region")},
    {"name": "avoid duplicate column names", "source": "AnalysisResultTest.scala:181-226", "tags": {"name": "EU"},
     "forAnalyzers": [], "withTags": [], "rows": rows(ALL, "name_2"), "json": expected_json(ALL, "name_2")},
    {"name": "only some specific tags", "source": "AnalysisResultTest.scala:228-277",
     "tags": {"Region": "EU", "Data Set Name": "Some"}, "forAnalyzers": [], "withTags": ["Region"],
     "rows": rows(ALL, "region"), "json": expected_json(ALL, "region")},
    {"name": "no entries", "source": "AnalysisResultTest.scala:279-313", "tags": {"Region": "EU"},
     "forAnalyzers": [], "withTags": [], "empty_context": True, "rows": [], "json": "[]"},
]

# SimpleResultSerdeTest (AnalysisResultSerdeTest.scala:197-234): the analysis over dfFull and its expected string
SIMPLE = [("Column", "att2", "Completeness", 1.0, {"analyzerName": "Completeness", "column": "att2"}),
          ("Column", "att1", "Completeness", 1.0, {"analyzerName": "Completeness", "column": "att1"}),
          ("Column", "att2", "Uniqueness", 0.25, {"analyzerName": "Uniqueness", "columns": ["att2"]}),
          ("Column", "item", "Distinctness", 1.0, {"analyzerName": "Distinctness", "columns": ["item"]}),
          ("Dataset", "*", "Size", 4.0, {"analyzerName": "Size"}),
          ("Column", "att1", "Uniqueness", 0.25, {"analyzerName": "Uniqueness", "columns": ["att1"]}),
          ("Column", "att1", "Distinctness", 0.5, {"analyzerName": "Distinctness", "columns": ["att1"]}),
          ("Mutlicolumn", "att1,att2", "MutualInformation", 0.5623351446188083,
           {"analyzerName": "MutualInformation", "columns": ["att1", "att2"]})]
simple_result_serde = {
    "source": "AnalysisResultSerdeTest.scala:197-234", "tags": {"Region": "EU"}, "dataSetDate": DATE_ONE,
    "context": [[a, dm(e, n, i, v)] for e, i, n, v, a in SIMPLE],
    "json": "[" + ",".join(f'{{"dataset_date":{DATE_ONE},"entity":"{e}","region":"EU","instance":"{i}","name":"{n}",'
                           f'"value":{v}}}' for e, i, n, v, _ in SIMPLE) + "]",
}

out = {
    "_comment": "generated by make_repository_kats.py; data only, see its docstring for the sources",
    "DATE_ONE": DATE_ONE,
    "serde_layout": serde_layout,
    "pattern_match_round_trip": {"source": "AnalysisResultSerdeTest.scala:96-120", "column": "patternRule1",
                                 "pattern": "Patterns.EMAIL", "metric": dm("Column", "PatternMatch", "ColumnA", 5.0)},
    "failed_metric_refused": {"source": "AnalysisResultSerdeTest.scala:122-144, AnalysisResultSerde.scala:486-487",
                              "message": "Unable to serialize failed metrics."},
    "context_dfFull": {"source": "AnalysisResultTest.scala:326-332, :50-55", "metricMap": context_dfFull},
    "analysis_result_cases": analysis_result_cases,
    "simple_result_serde": simple_result_serde,
}

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "repository_kats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)
