"""deequ_amd -- MI355X-native replacement of Deequ's fused single-pass metric scan.

The hot path (AnalysisRunner.runScanningAnalyzers / ScanShareableAnalyzer aggregation) runs in
libdqscan.so: hand-written gfx950 HIP kernels behind the C ABI in include/dqscan.h.  This package
is the host-side mirror of the reference's analyzer / state / runner API over that ABI.
"""
from ._lib import DQError, lib  # noqa: F401  (fails loudly if libdqscan.so is missing)
from .checks import (Check, CheckLevel, CheckStatus, ConstrainableDataTypes, ConstraintStatus,  # noqa: F401
                     VerificationResult, VerificationSuite)
from .checks import AnomalyCheckConfig, getAnomalyCheck  # noqa: F401
from .anomaly import (Anomaly, AnomalyDetectionStrategy, AnomalyDetector, BatchNormalStrategy, DataPoint,  # noqa: F401
                      DetectionResult, HistoryUtils, HoltWinters, OnlineNormalStrategy, RateOfChangeStrategy,
                      SimpleThresholdStrategy)
from .repository import (AnalysisResult, AnalysisResultSerde, FileSystemMetricsRepository,  # noqa: F401
                         InMemoryMetricsRepository, MetricsRepository, MetricsRepositoryMultipleResultsLoader,
                         ResultKey)
from .analyzers import (ApproxCountDistinct, Completeness, Compliance, Correlation, DataType,  # noqa: F401
                        DataTypeInstances, MaxLength, Maximum, Mean, MinLength, Minimum, PatternMatch, Patterns, Size,
                        StandardDeviation, Sum)
from .binning import Bins  # noqa: F401
from .lengths import string_lengths  # noqa: F401
from .grouping import (CountDistinct, Distinctness, Entropy, FrequenciesAndNumRows, Histogram,  # noqa: F401
                       MutualInformation, Uniqueness, UniqueValueRatio)
from .matching import DatasetMatch, KeyedRows, KeySet, ReferentialIntegrity  # noqa: F401
from .drift import DistributionDistance, ReferenceDistribution, StoredDistribution  # noqa: F401
from . import segments  # noqa: F401
from .segments import (SegmentedAnalyzerContext, SegmentedVerificationResult, run_segmented)  # noqa: F401
from .metrics import (DoubleMetric, Distribution, DistributionValue, Entity, HistogramMetric,  # noqa: F401
                      KeyedDoubleMetric)
from .profiles import (ColumnProfiler, ColumnProfilerRunBuilder, ColumnProfilerRunner, ColumnProfiles,  # noqa: F401
                       NumericColumnProfile, StandardColumnProfile,
                       compute_histograms)
from .quantiles import ApproxQuantile, ApproxQuantiles  # noqa: F401
from .runner import AnalysisRunner, AnalyzerContext, ReusingNotPossibleResultsMissingException  # noqa: F401
from .schema import (RowLevelSchema, RowLevelSchemaValidationResult, RowLevelSchemaValidator)  # noqa: F401
from .rowlevel import (RowLevelPlan, RowLevelResults, RowOutcome, plan_row_level, row_level_results)  # noqa: F401
from .split import random_split  # noqa: F401
from .suggestions import (ConstraintSuggestion, ConstraintSuggestionResult, ConstraintSuggestionRunner,  # noqa: F401
                          ConstraintSuggestions, Rules, UniqueIfApproximatelyUniqueRule)
from .state_provider import HdfsStateProvider, InMemoryStateProvider  # noqa: F401
from .states import (ApproxCountDistinctState, CorrelationState, DataTypeHistogram, MaxState, MeanState,  # noqa: F401
                     MinState, NumMatches, NumMatchesAndCount, StandardDeviationState, SumState)
from .table import Column, Table  # noqa: F401
