/* taudem_amd_sinmap.h - the SinmapSI part of the C ABI of libtaudem_amd.so.  Included by taudem_amd.h (inside its extern "C" block, after the
 * types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_SINMAP_H
#define TAUDEM_AMD_SINMAP_H

/* SinmapSI: sindexcombined() src/SinmapSI.cpp:138-441 and sindexcell() :449-551, the SINMAP stability index si and the saturation raster sat.
 * Rasters: slp float32 (tan of the slope angle, what dinfflowdir writes), sca float32 (specific catchment area, what areadinf writes), cal int16 (the
 * calibration region of a cell), scamin / scamax float32 (the road contributions; either may be NULL, and one that is absent counts as 0).
 * The region table is nreg entries of plain arrays, in the order of the -calpar file: reg_id, and tmin tmax cmin cmax phimin phimax rhos as the
 * floats the reference scans (phi in degrees).  A cell's region is the FIRST entry whose id equals its cal value; cal == (int16_t)cal_nodata, an id
 * that is not listed, and listed ids outside the int16 range never match.  rminter / rmaxter: the recharge bounds (the reference's floats, widened);
 * g is not used by the reference's formulas and is taken for the signature's sake; rhow / rhos is a float division.
 * Per cell: nodata (-1 in both outputs) when no region matches, sca < 0, scamin < 0, scamax < 0 or slp == slp_nodata; also -1 when rmaxter == 0 and
 * scamax == 0 (the reference leaves the cell at its initial value); otherwise si = (float)sindexcell(slp, 1, cmin, cmax, phimin, phimax, x1, x2, r,
 * &sat) with x2 = (sca * rmaxter + scamax) / tmin and x1 = (sca * rminter + scamin) / tmax, in double, in the reference's operation order.
 * tan(phi) and rhow / rhos are taken on the host with the host's libm, so those bits are the reference's; atan, sin, cos of the slope and the
 * logarithms of the integrals are the device's, which is why si is close to, not equal to, the reference's ("SinmapSI").
 * Cells are independent: the strip form (arrays of ny_local + 2 rows) computes its owned rows, exchanges nothing and leaves the halo rows of si and
 * sat unwritten.  comm may be NULL. */
int tdx_sinmapsi_dev(tdx_context* ctx, const float* d_slp, const float* d_sca, const float* d_scamin, const float* d_scamax, const int16_t* d_cal, int64_t nx,
                     int64_t ny, float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id, const float* tmin, const float* tmax, const float* cmin,
                     const float* cmax, const float* phimin, const float* phimax, const float* rhos, double rminter, double rmaxter, float g, float rhow, float* d_si,
                     float* d_sat, tdx_stats* stats);
int tdx_sinmapsi(tdx_context* ctx, const float* slp, const float* sca, const float* scamin, const float* scamax, const int16_t* cal, int64_t nx, int64_t ny,
                 float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id, const float* tmin, const float* tmax, const float* cmin, const float* cmax,
                 const float* phimin, const float* phimax, const float* rhos, double rminter, double rmaxter, float g, float rhow, float* si, float* sat,
                 tdx_stats* stats);
int tdx_sinmapsi_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_slp, const float* d_sca, const float* d_scamin, const float* d_scamax,
                       const int16_t* d_cal, int64_t nx, int64_t ny_local, float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id, const float* tmin,
                       const float* tmax, const float* cmin, const float* cmax, const float* phimin, const float* phimax, const float* rhos, double rminter,
                       double rmaxter, float g, float rhow, float* d_si, float* d_sat, tdx_stats* stats);
/* The -calpar text file: one header line, then one line "id,tmin,tmax,cmin,cmax,phimin,phimax,rhos" per region, scanned as the reference scans it
 * (%i for the id: 0x.. and leading-zero octal are taken; %f for the rest; blanks around the fields).  Blank lines after the last region are ignored.
 * Host only: no GPU, no context.  *count = the number of regions in the file; up to `capacity` of them are stored (reg_id and the seven float arrays
 * may be NULL with capacity 0 to ask for the count).  Returns 0; 15 when the file cannot be read (the reference's code); TDX_ERR_ARG for a data line
 * with fewer than 8 fields, with "line N" in tdx_last_error(NULL) (the reference reads uninitialised values there). */
int tdx_sinmap_read_calpar(const char* path, int32_t capacity, int32_t* reg_id, float* tmin, float* tmax, float* cmin, float* cmax, float* phimin, float* phimax,
                           float* rhos, int32_t* count);
/* int sindexcombined(char* slopefile, char* scaterrainfile, char* scarminroadfile, char* scarmaxroadfile, char* tergridfile, char* terparfile,
 *                    char* satfile, char* sincombinedfile, double Rminter, double Rmaxter, double* par)       src/SinmapSI.cpp:138   (par: g, rhow)
 * An empty road file name: that raster is absent. */
int tdx_tool_sinmapsi(const char* slopefile, const char* scaterrainfile, const char* scarminroadfile, const char* scarmaxroadfile, const char* tergridfile,
                      const char* terparfile, const char* satfile, const char* sincombinedfile, double rminter, double rmaxter, const double* par);

#endif /* TAUDEM_AMD_SINMAP_H */
