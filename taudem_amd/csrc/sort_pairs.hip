// Device radix sort of (key, uint32 value) pairs - rocPRIM through hipCUB; stable.  uint32 keys: once per AreaD8 call to put the few cells whose count
// exceeds 2^24 into dependency order (ascending count).  uint64 keys, the low end_bit bits of them: once per device link build of StreamNet, to put the
// cells that create links into the order the reference's queue pops them.  Neither is a hot operation.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "context.hpp"

namespace {
template <class K>
int sort_pairs(tdx_context* ctx, int scratch_slot, const K* keys_in, K* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n, int end_bit) {
    if (n == 0) return TDX_OK;
    size_t bytes = 0;
    TDX_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, int(n), 0, end_bit, ctx->stream));
    void* tmp = ctx->scratch(scratch_slot, bytes);
    if (!tmp) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, int(n), 0, end_bit, ctx->stream));
    return TDX_OK;
}
}  // namespace

int tdx_sort_pairs_u32(tdx_context* ctx, int scratch_slot, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                       size_t n) {
    return sort_pairs(ctx, scratch_slot, keys_in, keys_out, vals_in, vals_out, n, 32);
}

int tdx_sort_pairs_u64(tdx_context* ctx, int scratch_slot, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out,
                       size_t n, int end_bit) {
    return sort_pairs(ctx, scratch_slot, keys_in, keys_out, vals_in, vals_out, n, end_bit);
}
