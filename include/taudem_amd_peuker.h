/* taudem_amd_peuker.h - the PeukerDouglas part of the C ABI of libtaudem_amd.so.  Included by taudem_amd.h (inside its extern "C" block, after the
 * types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_PEUKER_H
#define TAUDEM_AMD_PEUKER_H

/* PeukerDouglas: peukerdouglas() src/PeukerDouglas.cpp:54-241, the stream-source raster whose weighted AreaD8 is the -ssa of DropAnalysis and Threshold.
 * fel is smoothed in float with the weights w_center, w_side, w_diag (the reference's -par, defaults 0.4 0.1 0.05): a cell on the raster's first or last
 * row or column, or a nodata cell, is copied; every other cell is (w_center*z + sum over the data neighbours of z_k*w) / (sum of the weights used),
 * sides 1 3 5 7 first, then diagonals 2 4 6 8, a group being skipped when its weight is not > 0.  Every smoothed cell starts flagged; each 2x2 group
 * of the smoothed grid then unflags its highest cell (the first one in the order x,y  x+1,y  x,y+1  x+1,y+1 under a strict '>'; the first cell starts
 * the maximum without a nodata test), every cell equal to that maximum, and all four cells when one of the last three is nodata.  The reference scans
 * the groups one after the other, but only ever clears flags: the result is the initial mask minus the union over the groups, computed per cell.
 * ss: int16, 1 = stream source, 0 elsewhere (the file's nodata value -2 is never written).  w (may be NULL): the same values as float32, which is what
 * tdx_aread8's weight raster takes.  Cell sizes are not used.  All values are exact: equal to the reference's output bit for bit.
 * The _dev form runs one fused pass (4 bytes read, 2 written per cell, + 4 with w); with TDX_PEUKER_TWOPASS set in the environment it runs the two
 * kernels of the strip form instead (an A/B hook).  The strip form (arrays of ny_local + 2 rows; it exchanges the halo rows of fel itself, which is
 * why fel is not const) smooths its owned rows into scratch, exchanges the smoothed edge rows - the two share() calls of the reference - and flags;
 * "first / last row" is the raster's: rank 0's first owned row and the last rank's last owned row.  comm == NULL: a single strip. */
int tdx_peukerdouglas_dev(tdx_context* ctx, const float* d_fel, int64_t nx, int64_t ny, float fel_nodata, float w_center, float w_side, float w_diag,
                          int16_t* d_ss, float* d_w, tdx_stats* stats);
int tdx_peukerdouglas(tdx_context* ctx, const float* fel, int64_t nx, int64_t ny, float fel_nodata, float w_center, float w_side, float w_diag, int16_t* ss,
                      float* w, tdx_stats* stats);
int tdx_peukerdouglas_strip(tdx_context* ctx, const tdx_comm* comm, float* d_fel, int64_t nx, int64_t ny_local, float fel_nodata, float w_center,
                            float w_side, float w_diag, int16_t* d_ss, float* d_w, tdx_stats* stats);
/* int peukerdouglas(char* felfile, char* ssfile, float* p)                  src/PeukerDouglas.cpp:54   (p: the three weights) */
int tdx_tool_peukerdouglas(const char* felfile, const char* ssfile, const float* p);

#endif /* TAUDEM_AMD_PEUKER_H */
