/* taudem_amd_outlets.h - the outlet tools of the C ABI of libtaudem_amd.so: MoveOutletsToStrm, ConnectDown and the point-layer writer they share.
 * Included by taudem_amd.h (inside its extern "C" block, after the types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_OUTLETS_H
#define TAUDEM_AMD_OUTLETS_H

/* MoveOutletsToStrm: the walk of src/MoveOutletsToStrm.cpp:370-435 on one rank.  p int16, src int32 (a stream cell has src not nodata and src >= 1).
 * Outlet i starts on column outlet_x[i], row outlet_y[i] (HOST lists, tiffIO::geoToGlobalXY of its coordinates) and walks down p until it stands on
 * a stream cell; dist_moved[i] is the number of steps, or -1 where the outlet could not be moved: it starts off the raster, it meets a p outside
 * 1..8 (nodata included) off the stream, its receiver lies off the raster, or it has walked maxdist steps without meeting the stream.  out_x / out_y
 * (HOST, n_outlets each) are the cell the outlet reached - with dist_moved == -1 the cell at which it gave up; the tool writes the original
 * coordinates then.  One lane per outlet on rasters that stay where they are: nothing of p or src is copied. */
int tdx_moveoutlets_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny, int16_t p_nodata, int32_t src_nodata, int32_t maxdist,
                        const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, int32_t* out_x, int32_t* out_y, int32_t* dist_moved, tdx_stats* stats);
int tdx_moveoutlets(tdx_context* ctx, const int16_t* p, const int32_t* src, int64_t nx, int64_t ny, int16_t p_nodata, int32_t src_nodata, int32_t maxdist,
                    const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, int32_t* out_x, int32_t* out_y, int32_t* dist_moved, tdx_stats* stats);
/* Row strips (arrays of ny_local + 2 rows, the strip's first owned row is row row0 of a raster of ny_total rows; no halo row is read).  The state
 * of every outlet - column, GLOBAL row, dist, done (0 / 1) - is HOST data the caller owns: the call advances every outlet that is not done and lies in
 * the strip's owned rows until it is done or has left them, and leaves the others alone.  The caller hands the state from strip to strip until a
 * round over all strips moves no outlet (*n_moved, may be NULL: the outlets this call advanced or finished).  Start with dist = 0, done = 0. */
int tdx_moveoutlets_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny_local, int64_t row0,
                          int64_t ny_total, int16_t p_nodata, int32_t src_nodata, int32_t maxdist, int32_t* state_x, int32_t* state_y, int32_t* state_dist,
                          int32_t* state_done, int64_t n_outlets, int64_t* n_moved, tdx_stats* stats);

/* ConnectDown: src/ConnectDown.cpp:177-247, :402-434 on one rank.  w int32 (every value that is not nodata is a watershed id), ad8 float32 (read
 * without a nodata test), p int16.  For every id, in ascending order: the cell of greatest ad8 (strict >, so the first cell in row-major order wins a
 * tie, -0.0 ties with +0.0, a NaN wins only as the id's first cell), then movedist steps down p from it (fewer where p leaves 1..8 or the raster);
 * id_down is w at the cell reached.  Ids are 0 .. TDX_CONNECTDOWN_MAX_ID: a negative id (the reference indexes its arrays with it) or a larger one is
 * refused with TDX_ERR_ARG.  The table behind the arg-max holds 8 bytes per id up to the largest one present.
 * The arg-max is one streaming pass over w and ad8 with one 64-bit atomic max per run of equal ids and wave.  *points is the caller's:
 * tdx_connectdown_points_free. */
#define TDX_CONNECTDOWN_MAX_ID 134217727 /* 2^27 - 1: a table of 1 GiB */
typedef struct tdx_connectdown_points tdx_connectdown_points;
int tdx_connectdown_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_w, const float* d_ad8, int64_t nx, int64_t ny, int16_t p_nodata, int32_t w_nodata,
                        int32_t movedist, tdx_connectdown_points** points, tdx_stats* stats);
int tdx_connectdown(tdx_context* ctx, const int16_t* p, const int32_t* w, const float* ad8, int64_t nx, int64_t ny, int16_t p_nodata, int32_t w_nodata,
                    int32_t movedist, tdx_connectdown_points** points, tdx_stats* stats);
int64_t tdx_connectdown_points_count(const tdx_connectdown_points* points);
/* ids, x, y (column and row of the maximum), ad8max, moved_x, moved_y, id_down: count values each; phase_ms [TDX_CONNECTDOWN_PHASES]: device
 * milliseconds of the call's phases (any may be NULL). */
#define TDX_CONNECTDOWN_MAXID 0   /* the reduction over w that sizes the table */
#define TDX_CONNECTDOWN_ARGMAX 1  /* the streaming pass over w and ad8 */
#define TDX_CONNECTDOWN_DECODE 2  /* table -> points in ascending id */
#define TDX_CONNECTDOWN_WALK 3    /* the walk down p */
#define TDX_CONNECTDOWN_PHASES 4
void tdx_connectdown_points_copy(const tdx_connectdown_points* points, int32_t* ids, int32_t* x, int32_t* y, float* ad8max, int32_t* moved_x, int32_t* moved_y,
                                 int32_t* id_down, double* phase_ms);
void tdx_connectdown_points_free(tdx_connectdown_points* points);
/* Row strips.  tdx_connectdown_strip: the arg-max of the strip's owned rows, with the table sized by the all-reduced maximum id; the points carry
 * GLOBAL rows and have not walked.  tdx_connectdown_merge (host code, no context): the parts of ALL strips in strip order -> the points of the
 * raster (a later strip wins with a strict >, which is row-major-first).  The walk of the merged points is tdx_connectdown_walk_strip, handed from
 * strip to strip like tdx_moveoutlets_strip (state_dist starts at 0; id_down is written by the strip that owns the last cell). */
int tdx_connectdown_strip(tdx_context* ctx, const tdx_comm* comm, const int32_t* d_w, const float* d_ad8, int64_t nx, int64_t ny_local, int64_t row0,
                          int32_t w_nodata, tdx_connectdown_points** part, tdx_stats* stats);
int tdx_connectdown_merge(const tdx_connectdown_points* const* parts, int64_t n_parts, tdx_connectdown_points** points);
int tdx_connectdown_walk_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_w, int64_t nx, int64_t ny_local, int64_t row0,
                               int64_t ny_total, int32_t movedist, int32_t* state_x, int32_t* state_y, int32_t* state_dist, int32_t* state_done,
                               int32_t* id_down, int64_t n_points, int64_t* n_moved, tdx_stats* stats);
/* The walked state into the merged points (moved_x, moved_y, id_down: count values each). */
int tdx_connectdown_points_set_moved(tdx_connectdown_points* points, const int32_t* moved_x, const int32_t* moved_y, const int32_t* id_down);

/* A point layer: ESRI shapefile (.shp with its .shx and .dbf) or GeoJSON (.json / .geojson), chosen by the extension of path; any other extension
 * is TDX_ERR_ARG.  types[i]: 0 Integer (columns[i]: int32_t*), 1 Real (double*), 2 String (const char* const*).  No .prj is written. */
int tdx_points_write(const char* path, const double* x, const double* y, int64_t n, int32_t nfields, const char* const* names, const int32_t* types,
                     const void* const* columns);

/* int outletstosrc(char *pfile, char *srcfile, char *outletsdatasrc, char *outletslayer, int uselyrname, int lyrno, char *outletmoveddatasrc,
 *                  char *outletmovedlayer, int maxdist)                                                            src/MoveOutletsToStrm.cpp:80
 * Every field of the outlet source is carried over and Dist_moved (Integer, width 6) appended.  The layer arguments are accepted and ignored. */
int tdx_tool_moveoutletstostrm(const char* pfile, const char* srcfile, const char* outletsdatasrc, const char* outletslayer, int uselyrname, int lyrno,
                               const char* outletmoveddatasrc, const char* outletmovedlayer, int maxdist);
/* int connectdown(char *pfile, char *wfile, char *ad8file, char *outletdatasrc, char *outletlyr, char *movedoutletdatasrc, char *movedoutletlyr,
 *                 int movedist)                                                                                       src/ConnectDown.cpp:79 */
int tdx_tool_connectdown(const char* pfile, const char* wfile, const char* ad8file, const char* outletdatasrc, const char* outletlyr,
                         const char* movedoutletdatasrc, const char* movedoutletlyr, int movedist);

#endif /* TAUDEM_AMD_OUTLETS_H */
