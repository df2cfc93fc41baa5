"""Metrics repository: store the metrics of a run under a key, load them back, query a history of runs.

Mirrors (paths relative to src/main/scala/com/amazon/deequ/repository/):
  MetricsRepository.scala:25-51                       MetricsRepository, ResultKey
  AnalysisResult.scala:25-137                         AnalysisResult, getSuccessMetricsAsJson / AsDataFrame
  MetricsRepositoryMultipleResultsLoader.scala:26-139 the loader and its json / rows union
  memory/InMemoryMetricsRepository.scala:28-136       InMemoryMetricsRepository
  fs/FileSystemMetricsRepository.scala:32-226         FileSystemMetricsRepository (a local path here)
  AnalysisResultSerde.scala:38-614                    the JSON layout, written the way Gson writes it

Everything here is host work on a handful of numbers per run: the metrics were computed by the GPU scan, the
repository only keeps them.  A DataFrame is a list of row dicts here (no Spark on this path).
"""
from __future__ import annotations

import json
import os
import re
import threading
import uuid
from typing import Dict, Iterable, List, Optional, Sequence

from .analyzers import (Analyzer, ApproxCountDistinct, Completeness, Compliance, Correlation, DataType, MaxLength, Maximum,
                        Mean, MinLength, Minimum, PatternMatch, Size, StandardDeviation, Sum)
from .grouping import (CountDistinct, Distinctness, Entropy, Histogram, MutualInformation, Uniqueness, UniqueValueRatio,
                       _java_double_to_string)
from .matching import DatasetMatch, ReferentialIntegrity, StoredKeyedRows, StoredKeySet
from .drift import DistributionDistance, StoredDistribution
from .metrics import (Distribution, DistributionValue, DoubleMetric, Entity, Failure, HistogramMetric,
                      KeyedDoubleMetric, MetricCalculationRuntimeException, Success)
from .quantiles import ApproxQuantile, ApproxQuantiles
from .runner import AnalyzerContext

DATASET_DATE_FIELD = "dataset_date"  # AnalysisResult.scala:32


class ResultKey:  # MetricsRepository.scala:51 (a case class: equal by dataSetDate and tags)
    __slots__ = ("dataSetDate", "tags")

    def __init__(self, dataSetDate: int, tags: Optional[Dict[str, str]] = None):
        self.dataSetDate = int(dataSetDate)
        self.tags: Dict[str, str] = dict(tags or {})

    def __eq__(self, other):
        return isinstance(other, ResultKey) and self.dataSetDate == other.dataSetDate and self.tags == other.tags

    def __hash__(self):
        return hash((self.dataSetDate, frozenset(self.tags.items())))

    def __repr__(self):
        tags = ", ".join(f"{k} -> {v}" for k, v in self.tags.items())
        return f"ResultKey({self.dataSetDate},Map({tags}))"


def _success_rows(context: AnalyzerContext, forAnalyzers: Sequence[Analyzer] = ()) -> List[dict]:
    """AnalyzerContext.successMetricsAsJson / successMetricsAsDataFrame with forAnalyzers
    (analyzers/runners/AnalyzerContext.scala:60-104): the flattened success metrics of the selected analyzers."""
    rows = []
    for analyzer, metric in context.metricMap.items():
        if forAnalyzers and analyzer not in forAnalyzers:
            continue
        for m in metric.flatten():
            if m.value.isSuccess:
                rows.append({"entity": m.entity.value, "instance": m.instance, "name": m.name, "value": m.value.get()})
    return rows


def _tag_column_name(tagName: str, taken: Iterable[str]) -> str:
    """formatTagColumnNameInDataFrame / InJson (AnalysisResult.scala:111-136)."""
    name = re.sub(r"[^A-Za-z0-9_]", "", tagName).lower()
    return name + "_2" if name in taken else name


class AnalysisResult:  # AnalysisResult.scala:25-137
    def __init__(self, resultKey: ResultKey, analyzerContext: AnalyzerContext):
        self.resultKey, self.analyzerContext = resultKey, analyzerContext

    def __eq__(self, other):
        return (isinstance(other, AnalysisResult) and self.resultKey == other.resultKey
                and self.analyzerContext.metricMap == other.analyzerContext.metricMap)

    def __repr__(self):
        return f"AnalysisResult({self.resultKey},{self.analyzerContext.metricMap})"

    @staticmethod
    def getSuccessMetricsAsDataFrame(analysisResult: "AnalysisResult", forAnalyzers: Sequence[Analyzer] = (),
                                     withTags: Sequence[str] = ()) -> List[dict]:  # :41-61
        """The rows form: dicts with the columns entity, instance, name, value, dataset_date, then one column per tag.
        A DataFrame keeps its columns without rows, a list of dicts does not: no success metric gives []."""
        rows = _success_rows(analysisResult.analyzerContext, forAnalyzers)
        columns = ["entity", "instance", "name", "value", DATASET_DATE_FIELD]
        for row in rows:
            row[DATASET_DATE_FIELD] = analysisResult.resultKey.dataSetDate
        for tagName, tagValue in analysisResult.resultKey.tags.items():
            if withTags and tagName not in withTags:
                continue
            # every name is formatted against the columns before any tag was added (:52-58), so two tags with one
            # formatted name land in one column and the later value stays
            column = _tag_column_name(tagName, columns)
            for row in rows:
                row[column] = tagValue
        return rows

    @staticmethod
    def getSuccessMetricsAsJson(analysisResult: "AnalysisResult", forAnalyzers: Sequence[Analyzer] = (),
                                withTags: Sequence[str] = ()) -> str:  # :70-92
        rows = _success_rows(analysisResult.analyzerContext, forAnalyzers)
        def add_column(column, value):  # addColumnToSerializableResult (:94-109): never overwrites
            if rows and column not in rows[0]:
                for row in rows:
                    row[column] = value

        add_column(DATASET_DATE_FIELD, analysisResult.resultKey.dataSetDate)
        taken = set(rows[0]) if rows else set()  # every tag name is formatted before the first tag is added (:83-89)
        named = [(_tag_column_name(tagName, taken), tagValue)
                 for tagName, tagValue in analysisResult.resultKey.tags.items()
                 if not withTags or tagName in withTags]
        for column, value in named:
            add_column(column, value)
        return SimpleResultSerde.serialize(rows)


class SimpleResultSerde:  # AnalysisResultSerde.scala:56-73
    @staticmethod
    def serialize(successData: Sequence[dict]) -> str:
        return _gson(list(successData), pretty=False, serialize_nulls=True)

    @staticmethod
    def deserialize(text: str) -> List[dict]:
        return [dict(row) for row in json.loads(text)]


class MetricsRepositoryMultipleResultsLoader:  # MetricsRepositoryMultipleResultsLoader.scala:26-96
    """The query over a repository's results.  after and before are both inclusive
    (InMemoryMetricsRepository.scala:121-122, FileSystemMetricsRepository.scala:137-138); withTagValues keeps a
    result whose tags contain every given pair."""

    def __init__(self):
        self._tagValues: Optional[Dict[str, str]] = None
        self._forAnalyzers: Optional[List[Analyzer]] = None
        self._before: Optional[int] = None
        self._after: Optional[int] = None

    def withTagValues(self, tagValues: Dict[str, str]) -> "MetricsRepositoryMultipleResultsLoader":
        self._tagValues = None if tagValues is None else dict(tagValues)
        return self

    def forAnalyzers(self, analyzers: Sequence[Analyzer]) -> "MetricsRepositoryMultipleResultsLoader":
        self._forAnalyzers = None if analyzers is None else list(analyzers)
        return self

    def after(self, dateTime: int) -> "MetricsRepositoryMultipleResultsLoader":
        self._after = dateTime
        return self

    def before(self, dateTime: int) -> "MetricsRepositoryMultipleResultsLoader":
        self._before = dateTime
        return self

    def _all(self) -> List[AnalysisResult]:
        raise NotImplementedError

    def get(self) -> List[AnalysisResult]:
        out = []
        for result in self._all():
            key = result.resultKey
            if self._after is not None and not self._after <= key.dataSetDate:
                continue
            if self._before is not None and not key.dataSetDate <= self._before:
                continue
            if self._tagValues is not None and not all(key.tags.get(k) == v and k in key.tags
                                                       for k, v in self._tagValues.items()):
                continue
            metrics = {a: m for a, m in result.analyzerContext.metricMap.items()
                       if self._forAnalyzers is None or a in self._forAnalyzers}
            out.append(AnalysisResult(key, AnalyzerContext(metrics)))
        return out

    def getSuccessMetricsAsDataFrame(self, withTags: Sequence[str] = ()) -> List[dict]:  # :64-79
        frames = [AnalysisResult.getSuccessMetricsAsDataFrame(r, withTags=withTags) for r in self.get()]
        columns: List[str] = []
        for frame in frames:  # dataFrameUnion (:122-131): every column of either side, None where one lacks it
            for column in (frame[0] if frame else ()):
                if column not in columns:
                    columns.append(column)
        return [{c: row.get(c) for c in columns} for frame in frames for row in frame]

    def getSuccessMetricsAsJson(self, withTags: Sequence[str] = ()) -> str:  # :82-95
        results = self.get()
        if not results:
            return AnalysisResult.getSuccessMetricsAsJson(AnalysisResult(ResultKey(0), AnalyzerContext.empty()))
        texts = [AnalysisResult.getSuccessMetricsAsJson(r, withTags=withTags) for r in results]
        acc = texts[0]
        for nxt in texts[1:]:
            acc = _json_union(acc, nxt)
        return acc


def _json_union(jsonOne: str, jsonTwo: str) -> str:  # MetricsRepositoryMultipleResultsLoader.scala:100-120
    one, two = SimpleResultSerde.deserialize(jsonOne), SimpleResultSerde.deserialize(jsonTwo)
    columns = list(one[0]) if one else []
    columns += [c for c in (two[0] if two else ()) if c not in columns]
    return SimpleResultSerde.serialize([{**row, **{c: None for c in columns if c not in row}} for row in two + one])


class MetricsRepository:  # MetricsRepository.scala:25-43
    def save(self, resultKey: ResultKey, analyzerContext: AnalyzerContext) -> None:
        raise NotImplementedError

    def loadByKey(self, resultKey: ResultKey) -> Optional[AnalyzerContext]:
        raise NotImplementedError

    def load(self) -> MetricsRepositoryMultipleResultsLoader:
        raise NotImplementedError


def _successful(analyzerContext: AnalyzerContext) -> AnalyzerContext:
    return AnalyzerContext({a: m for a, m in analyzerContext.metricMap.items() if m.value.isSuccess})


class _ListLoader(MetricsRepositoryMultipleResultsLoader):
    def __init__(self, source):
        super().__init__()
        self._source = source

    def _all(self):
        return self._source()


class InMemoryMetricsRepository(MetricsRepository):  # memory/InMemoryMetricsRepository.scala:28-63
    """Backed by a dict under a lock (the reference: a ConcurrentHashMap).  Only success metrics are stored."""

    def __init__(self):
        self._results: Dict[ResultKey, AnalysisResult] = {}
        self._lock = threading.Lock()

    def save(self, resultKey, analyzerContext):
        result = AnalysisResult(resultKey, _successful(analyzerContext))
        with self._lock:
            self._results[resultKey] = result

    def loadByKey(self, resultKey):
        with self._lock:
            result = self._results.get(resultKey)
        return None if result is None else result.analyzerContext

    def _snapshot(self) -> List[AnalysisResult]:
        with self._lock:
            return list(self._results.values())

    def load(self):
        return _ListLoader(self._snapshot)


class FileSystemMetricsRepository(MetricsRepository):  # fs/FileSystemMetricsRepository.scala:32-226
    """All results in one JSON file at a local path.  save reads the file, replaces the result under the key and
    writes a temporary file beside it that is renamed over it (writeToFileOnDfs, :167-196)."""

    CHARSET_NAME = "UTF-8"
    _lock = threading.Lock()

    def __init__(self, path: str):
        self.path = str(path)

    def _read(self) -> List[AnalysisResult]:
        if not os.path.isfile(self.path):  # readFromFileOnDfs (:199-216): no file, no results
            return []
        with open(self.path, "r", encoding=self.CHARSET_NAME) as f:
            return AnalysisResultSerde.deserialize(f.read())

    def save(self, resultKey, analyzerContext):
        with FileSystemMetricsRepository._lock:
            previous = [r for r in self._read() if r.resultKey != resultKey]
            text = AnalysisResultSerde.serialize(previous + [AnalysisResult(resultKey, _successful(analyzerContext))])
            directory = os.path.dirname(os.path.abspath(self.path))
            temp = os.path.join(directory, f"{uuid.uuid4()}.json")
            try:
                with open(temp, "x", encoding=self.CHARSET_NAME) as f:
                    f.write(text)
                os.replace(temp, self.path)
            finally:
                if os.path.exists(temp):
                    os.remove(temp)

    def loadByKey(self, resultKey):
        for result in self._read():
            if result.resultKey == resultKey:
                return result.analyzerContext
        return None

    def load(self):
        return _ListLoader(self._read)


# ----------------------------------------------------------------------------------------------- the JSON layout
_HTML_SAFE = {"<": "\\u003c", ">": "\\u003e", "&": "\\u0026", "=": "\\u003d", "'": "\\u0027",
              "\u2028": "\\u2028", "\u2029": "\\u2029"}


def _gson_string(s: str) -> str:
    """A string as Gson's JsonWriter writes it with its default htmlSafe setting."""
    out = json.dumps(s, ensure_ascii=False)
    return "".join(_HTML_SAFE.get(ch, ch) for ch in out)


def _gson(node, pretty: bool, serialize_nulls: bool = False, depth: int = 0) -> str:
    """A tree of dict / list / str / bool / int / float / None as Gson prints it: a double as java.lang.Double.toString
    (repr's shortest round-trip digits, so a value reads back bit for bit), NaN and +-Infinity as those bare words
    (Gson.toJson makes its writer lenient), a None member dropped unless serialize_nulls, and setPrettyPrinting's
    two-space layout when pretty."""
    if node is None:
        return "null"
    if node is True or node is False:
        return "true" if node else "false"
    if isinstance(node, str):
        return _gson_string(node)
    if isinstance(node, int):
        return str(node)
    if isinstance(node, float):
        return _java_double_to_string(node)
    nl = "\n" + "  " * (depth + 1) if pretty else ""
    end = "\n" + "  " * depth if pretty else ""
    if isinstance(node, dict):
        parts = [f"{_gson_string(str(k))}:{' ' if pretty else ''}{_gson(v, pretty, serialize_nulls, depth + 1)}"
                 for k, v in node.items() if v is not None or serialize_nulls]
        return "{" + nl + ("," + nl).join(parts) + end + "}" if parts else "{}"
    if isinstance(node, (list, tuple)):
        parts = [_gson(v, pretty, serialize_nulls, depth + 1) for v in node]
        return "[" + nl + ("," + nl).join(parts) + end + "]" if parts else "[]"
    raise TypeError(f"not a JSON value: {node!r}")


_WHERE_ANALYZERS = {"Completeness": Completeness, "Sum": Sum, "Mean": Mean, "Minimum": Minimum, "Maximum": Maximum,
                    "DataType": DataType, "ApproxCountDistinct": ApproxCountDistinct,
                    "StandardDeviation": StandardDeviation, "MinLength": MinLength, "MaxLength": MaxLength}
_COLUMNS_ANALYZERS = {"CountDistinct": CountDistinct, "Distinctness": Distinctness,
                      "MutualInformation": MutualInformation, "UniqueValueRatio": UniqueValueRatio,
                      "Uniqueness": Uniqueness}


def serialize_analyzer(analyzer: Analyzer) -> dict:  # AnalyzerSerializer (AnalysisResultSerde.scala:220-347)
    node = _serialize_analyzer(analyzer)
    # the grouping, histogram and quantile analyzers' filter: a "where" member only when one is set, so an unfiltered
    # analyzer's JSON is the reference's
    if "where" not in node and getattr(analyzer, "where", None) is not None:
        node["where"] = analyzer.where
    return node


def _serialize_analyzer(analyzer: Analyzer) -> dict:
    t = type(analyzer)
    if t is Size:
        return {"analyzerName": "Size", "where": analyzer.where}
    if t is Compliance:
        return {"analyzerName": "Compliance", "where": analyzer.where, "instance": analyzer.instance,
                "predicate": analyzer.predicate}
    if t is PatternMatch:
        return {"analyzerName": "PatternMatch", "column": analyzer.column, "where": analyzer.where,
                "pattern": analyzer.pattern}
    for name, cls in _WHERE_ANALYZERS.items():
        if t is cls:
            return {"analyzerName": name, "column": analyzer.column, "where": analyzer.where}
    if t is Entropy:
        return {"analyzerName": "Entropy", "column": analyzer.columns[0]}
    for name, cls in _COLUMNS_ANALYZERS.items():
        if t is cls:
            return {"analyzerName": name, "columns": list(analyzer.columns)}
    if t is Histogram:
        if analyzer.binningUdf is not None:
            raise ValueError("Unable to serialize Histogram with binningUdf!")
        node = {"analyzerName": "Histogram", "column": analyzer.column, "maxDetailBins": int(analyzer.maxDetailBins)}
        if analyzer.binning is not None:  # (no upstream layout; without a binning the JSON is the reference's)
            from .binning import bins_to_json

            node["binning"] = bins_to_json(analyzer.binning)
        return node
    if t is Correlation:
        return {"analyzerName": "Correlation", "firstColumn": analyzer.firstColumn,
                "secondColumn": analyzer.secondColumn, "where": analyzer.where}
    if t is ApproxQuantile:
        return {"analyzerName": "ApproxQuantile", "column": analyzer.column, "quantile": analyzer.quantile,
                "relativeError": analyzer.relativeError}
    if t is ApproxQuantiles:
        return {"analyzerName": "ApproxQuantiles", "column": analyzer.column,
                "quantiles": ",".join(_java_double_to_string(q) for q in analyzer.quantiles),
                "relativeError": analyzer.relativeError}
    if t is ReferentialIntegrity:
        # (no upstream layout: the analyzer postdates the serde this follows.)  The key set itself is not stored,
        # only its size: the analyzer comes back able to key stored metrics and refusing to run (StoredKeySet)
        return {"analyzerName": "ReferentialIntegrity", "columns": list(analyzer.columns), "where": analyzer.where,
                "numKeys": int(analyzer.reference.num_keys)}
    if t is DatasetMatch:
        # (no upstream layout either.)  The reference's rows are not stored, only its number of keys (StoredKeyedRows)
        return {"analyzerName": "DatasetMatch", "keyColumns": list(analyzer.keyColumns),
                "compareColumns": [[c, rc] for c, rc in analyzer.mapping or ()], "where": analyzer.where,
                "numKeys": int(analyzer.reference.num_keys)}
    if t is DistributionDistance:
        # (no upstream layout.)  The reference's table is not stored, only its numbers of groups and values
        # (StoredDistribution): the analyzer comes back able to key stored metrics and refusing to run
        from .binning import bins_to_json

        return {"analyzerName": "DistributionDistance", "columns": list(analyzer.columns), "method": analyzer.method,
                "where": analyzer.where,
                "binning": None if analyzer.binning is None else bins_to_json(analyzer.binning),
                "numGroups": int(analyzer.reference.num_groups), "numValues": int(analyzer.reference.num_values)}
    raise ValueError(f"Unable to serialize analyzer {analyzer}.")


def deserialize_analyzer(node: dict) -> Analyzer:  # AnalyzerDeserializer (:349-475)
    name = node["analyzerName"]
    where = node.get("where")
    if name == "Size":
        return Size(where)
    if name == "Compliance":
        return Compliance(node["instance"], node["predicate"], where)
    if name == "PatternMatch":
        return PatternMatch(node["column"], node["pattern"], where)
    if name in _WHERE_ANALYZERS:
        return _WHERE_ANALYZERS[name](node["column"], where)
    if name == "Entropy":
        return Entropy(node["column"], where)
    if name in _COLUMNS_ANALYZERS:
        return _COLUMNS_ANALYZERS[name](list(node["columns"]), where=where)
    if name == "Histogram":
        binning = None
        if node.get("binning") is not None:
            from .binning import bins_from_json

            binning = bins_from_json(node["binning"])
        return Histogram(node["column"], None, int(node["maxDetailBins"]), binning, where=where)
    if name == "Correlation":
        return Correlation(node["firstColumn"], node["secondColumn"], where)
    if name == "ApproxQuantile":
        return ApproxQuantile(node["column"], float(node["quantile"]), float(node["relativeError"]), where)
    if name == "ApproxQuantiles":
        return ApproxQuantiles(node["column"], [float(q) for q in node["quantiles"].split(",")],
                               float(node["relativeError"]), where)
    if name == "ReferentialIntegrity":
        return ReferentialIntegrity(list(node["columns"]), StoredKeySet(int(node["numKeys"])), where)
    if name == "DatasetMatch":
        return DatasetMatch(list(node["keyColumns"]), [tuple(m) for m in node["compareColumns"]],
                            StoredKeyedRows(int(node["numKeys"])), where)
    if name == "DistributionDistance":
        binning = None
        if node.get("binning") is not None:
            from .binning import bins_from_json

            binning = bins_from_json(node["binning"])
        return DistributionDistance(list(node["columns"]),
                                    StoredDistribution(int(node["numGroups"]), int(node["numValues"])),
                                    node["method"], binning, where)
    raise ValueError(f"Unable to deserialize analyzer {name}.")


def serialize_metric(metric) -> dict:  # MetricSerializer (:477-523), DistributionSerializer (:573-594)
    if metric.value.isFailure:
        raise ValueError("Unable to serialize failed metrics.")
    if isinstance(metric, DoubleMetric):
        return {"metricName": "DoubleMetric", "entity": metric.entity.value, "instance": metric.instance,
                "name": metric.name, "value": float(metric.value.get())}
    if isinstance(metric, HistogramMetric):
        d = metric.value.get()
        values = {key: {"absolute": int(v.absolute), "ratio": float(v.ratio)} for key, v in d.values.items()}
        return {"metricName": "HistogramMetric", "column": metric.column, "numberOfBins": int(d.numberOfBins),
                "value": {"numberOfBins": int(d.numberOfBins), "values": values}}
    if isinstance(metric, KeyedDoubleMetric):
        return {"metricName": "KeyedDoubleMetric", "entity": metric.entity.value, "instance": metric.instance,
                "name": metric.name, "value": {k: float(v) for k, v in metric.value.get().items()}}
    raise ValueError(f"Unable to serialize metrics {metric}.")


def deserialize_metric(node: dict):  # MetricDeserializer (:525-571), DistributionDeserializer (:596-614)
    name = node["metricName"]
    if name == "DoubleMetric":
        return DoubleMetric(Entity(node["entity"]), node["name"], node["instance"], Success(float(node["value"])))
    if name == "HistogramMetric":
        d = node["value"]
        values = {key: DistributionValue(int(v["absolute"]), float(v["ratio"])) for key, v in d["values"].items()}
        return HistogramMetric(node["column"], Success(Distribution(values, int(d["numberOfBins"]))))
    if name == "KeyedDoubleMetric":
        entity = Entity(node["entity"])
        if "value" in node:
            return KeyedDoubleMetric(entity, node["name"], node["instance"],
                                     Success({k: float(v) for k, v in node["value"].items()}))
        # the reference builds Failure(null) here; its serializer never writes a failed metric
        return KeyedDoubleMetric(entity, node["name"], node["instance"],
                                 Failure(MetricCalculationRuntimeException("null")))
    raise ValueError(f"Unable to deserialize analyzer {name}.")


class AnalysisResultSerde:  # AnalysisResultSerde.scala:75-106
    @staticmethod
    def serialize(analysisResults: Sequence[AnalysisResult]) -> str:
        tree = [{"resultKey": {"dataSetDate": r.resultKey.dataSetDate, "tags": dict(r.resultKey.tags)},
                 "analyzerContext": {"metricMap": [{"analyzer": serialize_analyzer(a), "metric": serialize_metric(m)}
                                                   for a, m in r.analyzerContext.metricMap.items()]}}
                for r in analysisResults]
        return _gson(tree, pretty=True)

    @staticmethod
    def deserialize(analysisResults: str) -> List[AnalysisResult]:
        out = []
        for node in json.loads(analysisResults):
            key = ResultKey(int(node["resultKey"]["dataSetDate"]), node["resultKey"].get("tags") or {})
            metrics = {deserialize_analyzer(e["analyzer"]): deserialize_metric(e["metric"])
                       for e in node["analyzerContext"]["metricMap"]}
            out.append(AnalysisResult(key, AnalyzerContext(metrics)))
        return out


def save_or_append_result(resultingAnalyzerContext: AnalyzerContext, metricsRepository: Optional[MetricsRepository],
                          saveOrAppendResultsWithKey: Optional[ResultKey]) -> None:
    """saveOrAppendResultsIfNecessary (analyzers/runners/AnalysisRunner.scala:195-213, VerificationSuite.scala:174-193):
    what is stored under the key ++ the new metrics; a new metric replaces a stored one of the same analyzer."""
    if metricsRepository is None or saveOrAppendResultsWithKey is None:
        return
    current = metricsRepository.loadByKey(saveOrAppendResultsWithKey) or AnalyzerContext.empty()
    metricsRepository.save(saveOrAppendResultsWithKey, current + resultingAnalyzerContext)
