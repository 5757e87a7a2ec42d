"""taudem_amd - MI355X (gfx950) implementation of TauDEM's D8 / D-infinity flow-direction and
contributing-area hot path (PitRemove -> D8FlowDir -> AreaD8, DinfFlowDir -> AreaDinf -> DinfDecayAccum).

Layers: ``csrc/`` hand-written HIP kernels + the C ABI of ``include/taudem_amd.h`` (libtaudem_amd.so);
``api`` in-memory binding (numpy host buffers or torch CUDA tensors); ``tools`` the reference's
file-level tool functions; ``dist`` row-strip multi-GPU orchestration over torch.distributed (RCCL).
"""
from ._lib import LIB_PATH, TdxError, load  # noqa: F401
from .api import (ANG_NODATA, AREA_NODATA, FEL_NODATA, P_NODATA, SLOPE_NODATA, Context, StreamNetLinks, catchhydrogeo, dropanalysis, dropanalysis_table, inundepth, peukerdouglas, raster_info, streamnet, streamnet_text,  # noqa: F401
                  read_raster, synth_base_wavelength, write_raster)
from .api import ConnectDownPoints, connectdown, moveoutletstostrm, write_points  # noqa: F401
from .api import read_calpar, sinmapsi  # noqa: F401
from .api import lengtharea, setregion, terrain_indices  # noqa: F401
from .api import editraster, read_changes  # noqa: F401
from .api import catchoutlets, read_lines, streamnet_net, write_lines  # noqa: F401
from .api import Polygons, polygonize  # noqa: F401
from .api import PackedPolygons, PolygonLayer, read_polygons, regiongrid, write_calpar  # noqa: F401

__version__ = "0.1.0"
