// StreamNet's link builder on the device (streamnet_links_device.hip): from the compact stream-cell columns that streamnet.hip's gather_kernel leaves in
// device memory to the tree and coord rows, which are all that is downloaded; the per-cell labels and orders stay on the device for the scatter.  It
// makes, byte for byte, what streamnet::build_links (streamnet_links.cpp: the default and the witness) makes of the same columns.
#pragma once
#include <cstdint>
#include <string>

#include "context.hpp"
#include "streamnet_links.hpp"

namespace streamnet {

enum { DLINK_CLASSIFY = 0, DLINK_JUMP, DLINK_LEVEL, DLINK_NUMBER, DLINK_LINKS, DLINK_ROWS, DLINK_DOWNLOAD, DLINK_PHASES };

struct DeviceLinkStats {
    double ms[DLINK_PHASES] = {0, 0, 0, 0, 0, 0, 0};   // wall milliseconds, each phase ended with the stream drained
    int64_t jump_rounds = 0;                             // pointer-jumping rounds along the cells with one inflow (at most ceil(log2(n)) + 1)
    int64_t level_rounds = 0;                            // rounds of the pass over the link tree (at most the number of cells where links start, + 1)
    int64_t workspace_bytes = 0;                         // scratch taken beside the columns, the coord rows included
};

// The columns in device memory of ctx, n cells in row-major order.  The raster index of cell i is idx64[i] where idx64 is not null, else cidx[i].
struct DeviceColumns {
    int64_t n = 0;
    const uint32_t* cidx = nullptr;
    const int64_t* idx64 = nullptr;
    const int16_t* p = nullptr;
    const float* fel = nullptr;
    const float* ad8 = nullptr;
    const float* len = nullptr;
    const int32_t* recv = nullptr;
    const uint8_t* flags = nullptr;
};

// Outlets: HOST lists as for tdx_streamnet.  d_label / d_order: n values each in device memory of ctx, written here.  out: tree and coord only (label
// and order stay empty).  TDX_OK; TDX_ERR_ARG (n >= 2^31, with the reason in err); TDX_ERR_NOMEM; TDX_ERR_HIP.
int build_links_device(tdx_context* ctx, const DeviceColumns& C, const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets,
                       int64_t nx, int64_t ny, double dxA, double dyA, const double* gt, int32_t* d_label, int16_t* d_order, Links& out, DeviceLinkStats& ds,
                       std::string& err);

}  // namespace streamnet
