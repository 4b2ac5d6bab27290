"""xmhw_amd -- MI355X (gfx950) implementation of xmhw's threshold() hot path and of its consumer.

    from xmhw_amd import threshold, detect     # same signatures as xmhw.xmhw.threshold / detect

The device side is hand-written HIP behind a C ABI (include/xmhw_amd.h); this
package holds only the host side of the path.  Importing it does not need a
GPU; calling threshold() does, and fails loudly without the HIP extension.
"""
from .exception import XmhwException
from .api import threshold, threshold_array, GridSeries, ClimDataset
from .calendar import add_doy, get_calendar
from .landmask import land_check
from .detect import detect, threshold_detect, EventDataset, InterDataset, climatology_series
from .device import release_device_cache
from .stats import block_average, BlockDataset
from .rank import mhw_rank
from .trend import mean_trend, TrendDataset
from .coverage import mhw_coverage, CoverageDataset
from .objects import mhw_objects, ObjectDataset
from .tracks import mhw_tracks, TrackDataset
from .track_intensity import mhw_track_intensity, TrackIntensityDataset
from .track_parts import mhw_track_parts, TrackPartsDataset
from .track_genealogy import mhw_track_genealogy, TrackGenealogyDataset
from .track_shape import mhw_track_shape, TrackShapeDataset, compactness
from .region_series import region_series, RegionSeriesDataset
from .days_by import mhw_days_by, ClassDaysDataset, classes_from_events
from .cooccurrence import mhw_cooccurrence, CooccurrenceDataset
from .displacement import mhw_displacement, displacement_offsets, DisplacementDataset, DisplacementTable
from .heat_stress import heat_stress, maximum_monthly_mean, degree_heating_weeks, HeatStressDataset, MonthlyMeanDataset
from .index_regression import index_regression, IndexRegressionDataset
from .composite import mhw_composite, CompositeDataset
from .lag_correlation import lag_correlation, LagCorrelationDataset
from .distribution import anomaly_distribution, DistributionDataset
from .spatial_correlation import spatial_correlation, SpatialCorrelationDataset
from .coarsen import coarsen, CoarsenInfo, calendar_windows
from .regrid import regrid, RegridInfo, axis_bounds, overlap_table
from .ingest import open_series, threshold_file
from .detrend import detrend, DetrendSpec, FitDataset

__all__ = ["threshold", "threshold_array", "GridSeries", "ClimDataset", "XmhwException",
           "add_doy", "get_calendar", "land_check", "detect", "threshold_detect", "EventDataset", "InterDataset",
           "climatology_series", "release_device_cache", "block_average", "BlockDataset", "mhw_rank", "mean_trend", "TrendDataset", "mhw_coverage",
           "CoverageDataset", "mhw_objects", "ObjectDataset", "mhw_tracks", "TrackDataset", "mhw_track_intensity",
           "TrackIntensityDataset", "mhw_track_parts", "TrackPartsDataset", "mhw_track_genealogy", "TrackGenealogyDataset",
           "mhw_track_shape", "TrackShapeDataset", "compactness", "region_series", "RegionSeriesDataset", "mhw_days_by", "ClassDaysDataset",
           "classes_from_events", "mhw_cooccurrence", "CooccurrenceDataset", "mhw_displacement", "displacement_offsets",
           "DisplacementDataset", "DisplacementTable", "heat_stress", "maximum_monthly_mean", "degree_heating_weeks",
           "HeatStressDataset", "MonthlyMeanDataset", "index_regression", "IndexRegressionDataset", "mhw_composite",
           "CompositeDataset", "lag_correlation", "LagCorrelationDataset", "anomaly_distribution",
           "DistributionDataset", "spatial_correlation", "SpatialCorrelationDataset", "coarsen", "CoarsenInfo",
           "calendar_windows", "regrid", "RegridInfo", "axis_bounds", "overlap_table", "open_series",
           "threshold_file", "detrend", "DetrendSpec", "FitDataset"]
__version__ = "0.1.0"
