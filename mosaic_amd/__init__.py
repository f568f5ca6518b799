"""mosaic_amd: MI355X-native engine for Mosaic's point-in-polygon chip-join hot path.

Product path: libmosaic_hip.so (mosaic_amd/csrc, HIP for gfx950) behind the C ABI in
include/mosaic_hip.h; this package is the host-side mirror of the reference's function surface.
"""
from ._native import IllegalStateException, MosaicError, NativeUnavailable  # noqa: F401
from .context import (BNGIndexSystem, ChipTable, GeometryTable, H3IndexSystem, LineChipTable, MosaicContext,  # noqa: F401
                      RowPathRequired, line_intersection_aggregate_host, line_intersects_aggregate_host)
from .analyzer import MosaicAnalyzer, NotEnoughGeometries  # noqa: F401
from .knn import CellIndex, SpatialKNN  # noqa: F401

__all__ = ["MosaicContext", "MosaicAnalyzer", "NotEnoughGeometries", "ChipTable", "LineChipTable", "line_intersects_aggregate_host", "line_intersection_aggregate_host", "GeometryTable", "CellIndex", "SpatialKNN", "H3IndexSystem", "BNGIndexSystem", "IllegalStateException",
           "MosaicError", "NativeUnavailable"]
