// The ring builder of the watershed polygons on the device (polygon_rings_device.hip): from the three edge columns that polygonize.hip leaves in device
// memory to the finished layer, which is all that is downloaded.  It makes, array for array, what polygons::build_rings (polygon_rings.cpp: the
// default and the witness) makes of the same edges.
#pragma once
#include <cstdint>
#include <string>

#include "context.hpp"
#include "polygon_rings.hpp"

namespace polygons {

enum { RING_SUCCESSOR = 0, RING_VALIDATE, RING_LABEL, RING_PER_RING, RING_RANK, RING_HOLES, RING_ORDER, RING_SCATTER, RING_PHASES };

struct DeviceRingStats {
    double ms[RING_PHASES] = {0, 0, 0, 0, 0, 0, 0, 0};   // wall milliseconds, each phase ended with the stream drained
    int64_t rounds = 0;                                    // jump rounds of the ring label (at most ceil(log2(E)) + 1)
    int64_t workspace_bytes = 0;                           // scratch taken beside the edge columns
    double download_ms = 0;                                // the finished layer to the host
};

// d_key ascending, d_next, d_id: n_edges values each, in device memory of ctx.  TDX_OK; TDX_ERR_ARG with the host builder's reason in err (nothing
// in out); TDX_ERR_NOMEM when the workspace does not fit (nothing written); TDX_ERR_HIP.
int build_rings_device(tdx_context* ctx, const int64_t* d_key, const int64_t* d_next, const int32_t* d_id, uint64_t n_edges, int64_t nx, int64_t ny,
                       Polygons& out, DeviceRingStats& rs, std::string& err);

}  // namespace polygons
