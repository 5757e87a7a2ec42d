/* taudem_amd_indices.h - the terrain-index part of the C ABI of libtaudem_amd.so: TWI, SlopeArea, SlopeAreaRatio, LengthArea and SetRegion.
 * Included by taudem_amd.h (inside its extern "C" block, after the types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_INDICES_H
#define TAUDEM_AMD_INDICES_H

/* TWI (twigrid() src/TWI.cpp:49), SlopeArea (slopearea() src/SlopeArea.cpp:52) and SlopeAreaRatio (atanbgrid() src/SlopeAreaRatio.cpp:49) in one
 * pass over slp and sca (float32): any of the outputs d_twi, d_sa, d_sar (float32, nodata -1) may be NULL, at least one is not.
 *   twi  -1 where sca or slp is nodata (|v - nodata| < 1e-5, linearpart::isNodata) or not (slp > 0 && sca > 0); else RN_float(ln(sca / slp)), the
 *        quotient a float division.
 *   sa   slp >= 0 && sca >= 0 (no nodata test; a NaN fails): RN_float(slp^m) * RN_float(sca^n), a float product; else -1.
 *   sar  -1 where sca is nodata; else slp / sca, a float division (a nodata slp flows through, sca == 0 gives inf or NaN).
 * ln and the powers are evaluated in double and rounded once: the correctly rounded float unless the exact value lies within 2^-40 (relative) of
 * a rounding boundary; a libm that keeps its 1-ulp bound is within 1 ulp per call of that ("Terrain indices").
 * Cells are independent: the strip form (arrays of ny_local + 2 rows) computes its owned rows, exchanges nothing and leaves the halo rows of the
 * outputs unwritten.  comm may be NULL. */
int tdx_terrain_indices_dev(tdx_context* ctx, const float* d_slp, const float* d_sca, int64_t nx, int64_t ny, float slp_nodata, float sca_nodata, float m, float n,
                            float* d_twi, float* d_sa, float* d_sar, tdx_stats* stats);
int tdx_terrain_indices(tdx_context* ctx, const float* slp, const float* sca, int64_t nx, int64_t ny, float slp_nodata, float sca_nodata, float m, float n, float* twi,
                        float* sa, float* sar, tdx_stats* stats);
int tdx_terrain_indices_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_slp, const float* d_sca, int64_t nx, int64_t ny_local, float slp_nodata,
                              float sca_nodata, float m, float n, float* d_twi, float* d_sa, float* d_sar, tdx_stats* stats);

/* LengthArea (lengtharea() src/LengthArea.cpp:51): ss int16 = (ad8 >= M * plen^y) where plen >= 0, -32768 elsewhere (the reference leaves those cells
 * at the partition's initial value).  plen float32; ad8 float32 as AreaD8 leaves it, converted to int32 per cell the way the reference's LONG read of
 * a float file does it (NaN -> 0, halves away from zero, clamped to the int32 range) and back to float for the comparison; plen^y is the correctly
 * rounded float as above and M * plen^y a float product. */
int tdx_lengtharea_dev(tdx_context* ctx, const float* d_plen, const float* d_ad8, int64_t nx, int64_t ny, float M, float y, int16_t* d_ss, tdx_stats* stats);
int tdx_lengtharea(tdx_context* ctx, const float* plen, const float* ad8, int64_t nx, int64_t ny, float M, float y, int16_t* ss, tdx_stats* stats);
int tdx_lengtharea_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_plen, const float* d_ad8, int64_t nx, int64_t ny_local, float M, float y,
                         int16_t* d_ss, tdx_stats* stats);

/* SetRegion (setregion() src/SetRegion.cpp:78): out int32 = region_id where gw (int32) is not nodata or p (int16) is not nodata; where both are, region_id
 * if a neighbour k = 1..8 on the raster has p not nodata, p > 0 and |p - k| == 4 (it drains into the cell), else -2147483647.
 * The strip form fills the halo rows of d_p (rows 0 and ny_local + 1) from the neighbouring strips, with p_nodata beyond the raster; gw needs no halo. */
int tdx_setregion_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_gw, int64_t nx, int64_t ny, int16_t p_nodata, int32_t gw_nodata, int32_t region_id,
                      int32_t* d_out, tdx_stats* stats);
int tdx_setregion(tdx_context* ctx, const int16_t* p, const int32_t* gw, int64_t nx, int64_t ny, int16_t p_nodata, int32_t gw_nodata, int32_t region_id, int32_t* out,
                  tdx_stats* stats);
int tdx_setregion_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, const int32_t* d_gw, int64_t nx, int64_t ny_local, int16_t p_nodata, int32_t gw_nodata,
                        int32_t region_id, int32_t* d_out, tdx_stats* stats);

/* int twigrid(char* slopefile, char* areafile, char* twifile)                      src/TWI.cpp:49
 * int slopearea(char* slopefile, char* scafile, char* safile, float* p)            src/SlopeArea.cpp:52        (p: m, n)
 * int atanbgrid(char* slopefile, char* areafile, char* atanbfile)                  src/SlopeAreaRatio.cpp:49
 * int lengtharea(char* plenfile, char* ad8file, char* ssfile, float* p)            src/LengthArea.cpp:51       (p: M, y)
 * int setregion(char* fdrfile, char* regiongwfile, char* newfile, int32_t regionID)  src/SetRegion.cpp:78
 * The first four return 1 without a word for a second raster of another size; SetRegion says "File sizes do not match" and returns 5. */
int tdx_tool_twi(const char* slopefile, const char* areafile, const char* twifile);
int tdx_tool_slopearea(const char* slopefile, const char* scafile, const char* safile, const float* p);
int tdx_tool_slopearearatio(const char* slopefile, const char* areafile, const char* atanbfile);
int tdx_tool_lengtharea(const char* plenfile, const char* ad8file, const char* ssfile, const float* p);
int tdx_tool_setregion(const char* fdrfile, const char* regiongwfile, const char* newfile, int32_t region_id);

#endif /* TAUDEM_AMD_INDICES_H */
