/* taudem_amd_dropan.h - the DropAnalysis part of the C ABI of libtaudem_amd.so.  Included by taudem_amd.h (inside its extern "C" block, after the
 * types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_DROPAN_H
#define TAUDEM_AMD_DROPAN_H

/* DropAnalysis: dropan() src/DropAnalysis.cpp:172-705, which picks the threshold that tdx_threshold is run with.  For each of nthresh thresholds of the
 * ladder thresh_min .. thresh_max (steptype 0: log steps, else arithmetic; computed in float as the reference does; nthresh < 2 is refused) the
 * stream mask ssa >= thresh is ordered by the reference's own order rule (src/DropAnalysis.cpp:113-166, a scan over the inflows in neighbour order,
 * not textbook Strahler) and the elevation drops of its streams are collected.  All result arrays are HOST arrays of nthresh entries: thresh,
 * n1 / n2 (first-order / higher-order drops), sums [nthresh][4] = sum and sum of squares of the first-order drops, then of the higher-order drops
 * (fp64, added in a fixed order: the same input gives the same bits; each term is the reference's float drop, its square the float square), length
 * (the stream length, from integer per-row link counts and dxc / dyc in row order).  total_area: the float sum of ad8 over the outlets (HOST column
 * / row lists, file order) whose downstream neighbour has ssa nodata or <= 0, times dxA * dyA; outlets outside the raster are skipped, an outlet on
 * a cell without a direction 0..8 is refused with TDX_ERR_ARG.  optimum / found: the first threshold whose |t| < 2 (tdx_dropanalysis_table), 0 / 0
 * when there is none; table (may be NULL): the text of the table file, as tdx_dropanalysis_table writes it.  ssa is any raster that increases downstream (ad8 itself serves); p / ssa carry their nodata values, ad8 and fel are read
 * without a nodata test, as in the reference.  The float sums and the double length of the reference depend on the order its queue pops the
 * cells in: they are matched within rounding, everything else exactly.
 * grid_th, order, elevout: a test hook - when order / elevout are not NULL they receive the order (int16, nodata -32768) and the start elevation
 * carried down the stream (float, nodata -FLT_MAX) of every cell after threshold number grid_th.
 * The strip form (arrays of ny_local + 2 rows, dxc / dyc of those rows; it exchanges the halo rows of p, fel and ssa itself) returns the STRIP's n1 /
 * n2 / sums / length and outlet_term[n_outlets], ad8 of the strip's terminal outlets and 0 for every other one: the caller adds the strips in strip
 * order and the outlet terms in file order, and makes the optimum with tdx_dropanalysis_table. */
int tdx_dropanalysis_dev(tdx_context* ctx, const float* d_ad8, const int16_t* d_p, const float* d_fel, const float* d_ssa, int64_t nx, int64_t ny,
                         int16_t p_nodata, float ssa_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const int32_t* outlet_x,
                         const int32_t* outlet_y, int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype, int64_t grid_th,
                         int16_t* d_order, float* d_elevout, float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length, float* total_area,
                         float* optimum, int32_t* found, char* table, int64_t table_cap, tdx_stats* stats);
int tdx_dropanalysis(tdx_context* ctx, const float* ad8, const int16_t* p, const float* fel, const float* ssa, int64_t nx, int64_t ny, int16_t p_nodata,
                     float ssa_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const int32_t* outlet_x, const int32_t* outlet_y,
                     int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype, int64_t grid_th, int16_t* order, float* elevout,
                     float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length, float* total_area, float* optimum, int32_t* found,
                     char* table, int64_t table_cap, tdx_stats* stats);
int tdx_dropanalysis_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_ad8, int16_t* d_p, float* d_fel, float* d_ssa, int64_t nx,
                           int64_t ny_local, int16_t p_nodata, float ssa_nodata, const double* dxc, const double* dyc, const int32_t* outlet_x,
                           const int32_t* outlet_row, int64_t n_outlets, float thresh_min, float thresh_max, int64_t nthresh, int steptype,
                           int64_t grid_th, int16_t* d_order, float* d_elevout, float* thresh, int64_t* n1, int64_t* n2, double* sums, double* length,
                           float* outlet_term, tdx_stats* stats);
/* The table file and the console lines of DropAnalysis (src/DropAnalysis.cpp:597-674) from the FLOAT sums of all thresholds, with the reference's
 * own float / double expressions: pure host code, no context.  table / console (either may be NULL) receive NUL-terminated text; a buffer that is
 * too small is TDX_ERR_ARG (256 bytes per threshold + 512 are enough).  A row is written when n1 > 1 and n2 > 1; the optimum is the first
 * threshold with |t| < 2 (a NaN t never qualifies); when there is none, optimum = 0, found = 0 and the last line says 0.000000. */
int tdx_dropanalysis_table(int64_t nthresh, const float* thresh, const int64_t* n1, const int64_t* n2, const float* s1, const float* s1sq, const float* s2,
                           const float* s2sq, const double* length, float total_area, char* table, int64_t table_cap, char* console, int64_t console_cap,
                           float* optimum, int32_t* found);
/* int dropan(char* areafile, char* dirfile, char* elevfile, char* ssafile, char* dropfile, char* datasrc, char* lyrname, int uselyrname, int lyrno,
 *            float threshmin, float threshmax, int nthresh, int steptype, float* threshopt)                  src/DropAnalysis.cpp:172
 * (*threshopt: 0 when no threshold qualifies; may be NULL) */
int tdx_tool_dropanalysis(const char* areafile, const char* dirfile, const char* elevfile, const char* ssafile, const char* dropfile, const char* datasrc,
                          const char* lyrname, int uselyrname, int lyrno, float threshmin, float threshmax, int nthresh, int steptype, float* threshopt);

#endif /* TAUDEM_AMD_DROPAN_H */
