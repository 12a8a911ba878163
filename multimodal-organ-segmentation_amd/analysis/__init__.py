"""--mode analysis: SUV statistics, TMTV / TLG and SUV histograms over a PET volume and its predicted mask, computed
by csrc/analysis.hip from the files' raw voxel blocks (DESIGN.md "Analysis")."""
from .core import CaseRecord, analyze_files, analyze_raw, find_file, median_from_pair, voxel_volume_ml, write_csv
from .histogram import HistogramAnalyzer, histogram_results
from .run import analysis_config, run_analysis
from .suv import SUV_COLUMNS, SUVAnalyzer, organ_rows, tumor_result
from .tmtv import TMTVAnalyzer, tmtv_results

__all__ = ["SUVAnalyzer", "TMTVAnalyzer", "HistogramAnalyzer", "CaseRecord", "analyze_files", "analyze_raw",
           "find_file", "median_from_pair", "voxel_volume_ml", "write_csv", "organ_rows", "tumor_result",
           "tmtv_results", "histogram_results", "SUV_COLUMNS", "analysis_config", "run_analysis"]
