/* taudem_amd_regions.h - the SINMAP parameter region grid in the C ABI of libtaudem_amd.so: the toolbox step "Create Parameter Region Grid"
 * (pyfiles/SIRegionTool.py: one region everywhere, gdal.RasterizeLayer of a polygon layer by an attribute, or gdal.Warp of an existing region grid
 * by nearest neighbour).  Included by taudem_amd.h (inside its extern "C" block, after the types tdx_context, tdx_comm and tdx_stats): include that
 * header, not this one.
 *
 * The output raster is nx x ny, int16, nodata 0; gt are the six numbers of the DEM's geotransform, gt[2] and gt[4] must be 0.  A vertex (x, y) has the
 * pixel coordinates px = (x - gt[0]) / gt[1], py = (y - gt[3]) / gt[5]; cell (c, r) has its centre at xc = c + 0.5, yc = r + 0.5.  All arithmetic
 * is IEEE double in exactly the written order, nothing contracted into an FMA, nothing reassociated.
 *
 * Polygon mode.  A feature is a list of rings; every ring counts, outer rings and holes are not told apart.  A ring whose last vertex differs from
 * its first is closed implicitly; a ring of fewer than 3 distinct vertices is ignored.  An edge (px1, py1) - (px2, py2) crosses the scanline of row r
 * iff min(py1, py2) <= yc < max(py1, py2) (a horizontal edge never does; a vertex on a scanline counts once for a passing boundary and zero or two
 * times for a local extremum), at xs = px1 + (yc - py1) * (px2 - px1) / (py2 - py1).  Cell (c, r) is inside the feature iff the number of crossings
 * of row r with xs < xc is odd (an edge through a cell centre has that cell to its right).  The cell's value is the value of the LAST feature in
 * layer order that it is inside, 0 if there is none.  Values lie in 1 .. 32767 (sinmapsi reads the grid as int16 and 0 is nodata); any other value is
 * TDX_ERR_ARG naming the feature, before anything is launched.  Whether this cell-centre rule agrees with GDAL's filled-polygon scanline rule in
 * every tie is NOT verified: no GDAL was at hand.
 *
 * Resample mode.  The source is int32 with its own nodata and an unrotated geotransform sgt.  Cell (c, r): x = gt[0] + (c + 0.5) * gt[1],
 * y = gt[3] + (r + 0.5) * gt[5], sc = floor((x - sgt[0]) / sgt[1]), sr = floor((y - sgt[3]) / sgt[5]); it takes the source value if (sc, sr) is
 * on the source and the value is not the source's nodata, else 0.  Taken values outside 1 .. 32767 fail the call with TDX_ERR_ARG and their count
 * (a counting pass runs first: the output is not touched then).  No reprojection: both transforms are taken to be in one coordinate system.
 *
 * Constant mode.  Every cell is 1 (the script does not mask by the DEM's nodata; neither does this).
 *
 * Every mode returns the sorted values other than 0 that occur in the output (ids: room for TDX_REGIONGRID_MAX_IDS values; n_ids), gathered in the
 * pass that writes the raster: one presence bitmap of 32768 bits.  The same bytes on every run: the only atomics are xor, max and or on integers.
 *
 * The polygons: x, y [vertices]; ring_first [n_rings + 1] (the vertices of a ring); feature_first [n_features + 1] (the rings of a feature);
 * values [n_features]; all HOST arrays in every form.  workspace_words bounds the 32-bit words of parity bitmap a batch of features may take
 * (0: the default, 16 Mi words; a feature larger than the bound is a batch of its own).  phase_ms [TDX_REGIONGRID_PHASES] (may be NULL): wall
 * milliseconds of the phases, each ended with the stream drained - with NULL nothing is drained between the batches' kernels; workspace_bytes (may
 * be NULL): device bytes the call used besides the output.
 *
 * Numbers that are not finite.  A vertex whose pixel coordinates are not finite (a NaN or an infinity in the layer, a coordinate that overflows
 * in the division) is TDX_ERR_ARG naming the feature, before anything is launched.  With finite vertices xs can still come out infinite or NaN
 * where x2 - x1 or the product overflows; the rule above then holds as written: xs < xc is true for -inf and false for +inf and for NaN. */
#ifndef TAUDEM_AMD_REGIONS_H
#define TAUDEM_AMD_REGIONS_H

#define TDX_REGIONGRID_MAX_IDS 32767
#define TDX_REGIONGRID_PREPARE 0  /* host: edges in pixel coordinates, rows per edge and their scan, boxes, batches; the upload */
#define TDX_REGIONGRID_CROSS 1    /* one thread per (edge, row): the crossing toggles its bit */
#define TDX_REGIONGRID_FILL 2     /* prefix xor along the bitmap rows; inside bits raise the winner words */
#define TDX_REGIONGRID_WRITE 3    /* winner -> int16 value, the presence bitmap, its read-back (resample: the counting pass and the gather) */
#define TDX_REGIONGRID_PHASES 4

/* d_out: nx * ny int16 on the device (host form: out on the host) */
int tdx_regiongrid_dev(tdx_context* ctx, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first,
                       const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx, int64_t ny, int16_t* d_out,
                       int32_t* ids, int32_t* n_ids, double* phase_ms, int64_t* workspace_bytes, tdx_stats* stats);
int tdx_regiongrid(tdx_context* ctx, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first,
                   const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx, int64_t ny, int16_t* out, int32_t* ids,
                   int32_t* n_ids, double* phase_ms, int64_t* workspace_bytes, tdx_stats* stats);
/* Row strips: d_out is an array of ny_local + 2 rows whose row 1 is row row0 of a raster of ny_total rows (gt is the whole raster's).  The owned rows
 * are computed; nothing is exchanged and the halo rows are left unwritten.  comm is taken like every strip call takes it and is not used (NULL is
 * fine).  ids are those of the owned rows. */
int tdx_regiongrid_strip(tdx_context* ctx, const tdx_comm* comm, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings,
                         const int64_t* feature_first, const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx,
                         int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out, int32_t* ids, int32_t* n_ids, double* phase_ms,
                         int64_t* workspace_bytes, tdx_stats* stats);

/* Resample mode.  src: snx * sny int32, on the side of the output (a strip holds the WHOLE source on its device). */
int tdx_regiongrid_resample_dev(tdx_context* ctx, const int32_t* d_src, int64_t snx, int64_t sny, const double* sgt, int32_t src_nodata, const double* gt,
                                int64_t nx, int64_t ny, int16_t* d_out, int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats);
int tdx_regiongrid_resample(tdx_context* ctx, const int32_t* src, int64_t snx, int64_t sny, const double* sgt, int32_t src_nodata, const double* gt,
                            int64_t nx, int64_t ny, int16_t* out, int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats);
int tdx_regiongrid_resample_strip(tdx_context* ctx, const tdx_comm* comm, const int32_t* d_src, int64_t snx, int64_t sny, const double* sgt,
                                  int32_t src_nodata, const double* gt, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out,
                                  int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats);

/* Constant mode: every cell 1, ids = {1}. */
int tdx_regiongrid_constant_dev(tdx_context* ctx, int64_t nx, int64_t ny, int16_t* d_out, int32_t* ids, int32_t* n_ids, tdx_stats* stats);
int tdx_regiongrid_constant(tdx_context* ctx, int64_t nx, int64_t ny, int16_t* out, int32_t* ids, int32_t* n_ids, tdx_stats* stats);
int tdx_regiongrid_constant_strip(tdx_context* ctx, const tdx_comm* comm, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out,
                                  int32_t* ids, int32_t* n_ids, tdx_stats* stats);

/* The region parameter table of sinmapsi -calpar (host code, no context): the line "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens", then one
 * line "id,tmin,...,soildens" per id in the order given, the seven texts written as they are.  TDX_ERR_FILE: the file cannot be written. */
int tdx_regiongrid_write_calpar(const char* path, const int32_t* ids, int32_t n_ids, const char* const* seven_texts);

/* A polygon layer read from a file (host code, no context): ESRI shapefile of shape type 5, 15 or 25 (Z and M ignored, a null shape is a feature
 * without rings) with the .dbf beside it, or GeoJSON Polygon / MultiPolygon features in document order with their properties.  Every part becomes a
 * ring; nesting is not rebuilt.  TDX_ERR_ARG: an extension no reader exists for; TDX_ERR_FILE: a file that cannot be read, or whose headers, record
 * lengths, counts, part indices or .dbf record count lie.  *layer is the caller's: tdx_polygon_layer_free. */
typedef struct tdx_polygon_layer tdx_polygon_layer;
int tdx_polygon_layer_read(const char* path, tdx_polygon_layer** layer);
/* Number of features; *n_rings, *n_vertices, *n_fields may be NULL. */
int64_t tdx_polygon_layer_count(const tdx_polygon_layer* layer, int64_t* n_rings, int64_t* n_vertices, int64_t* n_fields);
/* feature_first [features + 1] (the rings of a feature), ring_first [rings + 1], x, y [vertices] (any may be NULL) */
void tdx_polygon_layer_copy(const tdx_polygon_layer* layer, int64_t* feature_first, int64_t* ring_first, double* x, double* y);
/* The name of field k and the text of a feature's value of it ("" is a null; a .dbf's bytes keep their padding); NULL when out of range. */
const char* tdx_polygon_layer_field(const tdx_polygon_layer* layer, int64_t k);
const char* tdx_polygon_layer_value(const tdx_polygon_layer* layer, int64_t feature, int64_t k);
/* The region ids: the integer values of `field`, one per feature (values may be NULL: the check alone).  TDX_ERR_ARG naming the feature: no such
 * field, the field name FID, a null, a value that is no integer, a value outside 1 .. 32767. */
int tdx_polygon_layer_values(const tdx_polygon_layer* layer, const char* field, int32_t* values);
void tdx_polygon_layer_free(tdx_polygon_layer* layer);

/* Create Parameter Region Grid: demfile gives the grid; shpfile (with shp_att_name, "ID" when NULL or empty) or parreg_infile (read as int32 with its
 * nodata value) give the regions, neither gives one region; parregfile: int16 GeoTIFF, nodata 0, the DEM's geotransform and geokeys; attfile: the
 * region table with one line per id that occurs.  Refused with TDX_ERR_ARG before anything is read: both sources, an output directory that does not
 * exist, a polygon source with an extension no reader exists for. */
int tdx_tool_siregiontool(const char* demfile, const char* parregfile, const char* attfile, const char* parreg_infile, const char* shpfile,
                          const char* shp_att_name, const char* const* seven_texts);

#endif /* TAUDEM_AMD_REGIONS_H */
