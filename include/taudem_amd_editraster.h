/* taudem_amd_editraster.h - the EditRaster part of the C ABI of libtaudem_amd.so.
 * Included by taudem_amd.h (inside its extern "C" block, after the types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_EDITRASTER_H
#define TAUDEM_AMD_EDITRASTER_H

/* EditRaster (editraster() src/EditRaster.cpp:69-168): out int16 = -32768 where in (int16) equals in_nodata, in elsewhere; then change k = 0 .. n - 1
 * sets the cell in column cols[k], row rows[k] to vals[k].  cols, rows, vals are HOST lists (int32), the cells tiffIO::geoToGlobalXY gives for the
 * points of the change file (tdx_outlets_to_cells).  A change off the raster is skipped, as the reference skips it; of several changes of one cell the
 * LAST one holds, as in the reference, which applies them in file order.  A value outside -32768 .. 32767 is refused with TDX_ERR_ARG before anything
 * is written (the reference scans "%d" into a short there and overwrites two bytes of its neighbour).
 * One streaming copy-and-recode pass over the raster, then one lane per change.  Which change of a cell holds is settled on the HOST before the
 * upload - the last one per cell is kept - so that the scatter has one writer per cell and needs no ordering on the device.
 * d_out == d_in is allowed: every cell is read and written by one lane, and the scatter runs after the pass in stream order.  The two arrays must
 * not overlap in any other way.
 * The strip form (arrays of ny_local + 2 rows; row0: the global row of the strip's first owned row) takes the same lists with GLOBAL rows, applies
 * the changes that fall in its owned rows, exchanges nothing and leaves the halo rows of d_out unwritten.  comm may be NULL. */
int tdx_editraster_dev(tdx_context* ctx, const int16_t* d_in, int64_t nx, int64_t ny, int16_t in_nodata, const int32_t* cols, const int32_t* rows, const int32_t* vals,
                       int64_t n, int16_t* d_out, tdx_stats* stats);
int tdx_editraster(tdx_context* ctx, const int16_t* in, int64_t nx, int64_t ny, int16_t in_nodata, const int32_t* cols, const int32_t* rows, const int32_t* vals, int64_t n,
                   int16_t* out, tdx_stats* stats);
int tdx_editraster_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_in, int64_t nx, int64_t ny_local, int64_t row0, int16_t in_nodata, const int32_t* cols,
                         const int32_t* rows, const int32_t* vals, int64_t n, int16_t* d_out, tdx_stats* stats);

/* The change file (src/EditRaster.cpp:124-133): the first line is skipped whatever it holds (at most 4096 characters of it), then "x,y,value" records are
 * scanned with "%lf,%lf,%d" until one does not scan - reading stops there without a word, and valid lines after it are not looked at.  Host code, no context.
 * x, y, vals: room for `capacity` records each (may be NULL with capacity 0); *n: the number of records in the file, of which the first
 * min(*n, capacity) have been stored.  TDX_ERR_FILE: the file cannot be opened.  TDX_ERR_ARG: a value outside -32768 .. 32767 - *n is then the index of
 * that record, and the records before it have been stored. */
int tdx_editraster_read_changes(const char* path, int64_t capacity, double* x, double* y, int32_t* vals, int64_t* n);

/* int editraster(char *rasterfile, char *newfile, char *changefile)                 src/EditRaster.cpp:69
 * The raster is read as int16 and written as int16 with the nodata tag -32768 and the input's georeferencing; per applied change, duplicates included,
 * the reference's line "Process: 0 changing x, y, value" is printed in file order. */
int tdx_tool_editraster(const char* rasterfile, const char* newfile, const char* changefile);

#endif /* TAUDEM_AMD_EDITRASTER_H */
