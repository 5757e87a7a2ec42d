/* taudem_amd_ad8.h - diagnostics of AreaD8's tile-contraction path in the C ABI of libtaudem_amd.so.  Included by taudem_amd.h (inside its extern "C"
 * block, after the type tdx_context): include that header, not this one. */
#ifndef TAUDEM_AMD_AD8_H
#define TAUDEM_AMD_AD8_H

/* The 64 x 64 tiles of the last AreaD8 call on this context that took the tile-contraction path (tdx_aread8, _dev, _strip without weights: this strip's
 * tiles; with outlets too, on the re-coded direction grid, where every tile that holds a cell outside the outlets' catchments is a redone one):
 * fast_tiles were counted by pointer doubling - all 64 rows valid, the tile and the ring of cells around it inside the array, every code there
 * 1 .. 8, no cycle -, redone_tiles by the Kahn sweep.  With TDX_AD8_LOCAL=kahn in the environment every tile is a redone one.  A call that takes
 * another path (weights, TDX_AD8_WALK, TDX_AD8_SWEEP) leaves the counters as they were.  Both 0 before the first such call. */
void tdx_context_ad8_tile_counters(const tdx_context* ctx, int64_t* fast_tiles, int64_t* redone_tiles);

#endif /* TAUDEM_AMD_AD8_H */
