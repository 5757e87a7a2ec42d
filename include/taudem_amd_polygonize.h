/* taudem_amd_polygonize.h - watershed polygons in the C ABI of libtaudem_amd.so: the toolbox step "Watershed Grid To Shapefile"
 * (pyfiles/WatershedGridToShapefile.py: RasterToPolygon_conversion(w, shp, "NO_SIMPLIFY", "Value")).  Included by taudem_amd.h (inside its extern "C"
 * block, after the types tdx_context, tdx_comm and tdx_stats): include that header, not this one.
 *
 * w is int32; every value that is not w_nodata is an id, negative values and 0 included.  Vertex (c, r) has 0 <= c <= nx, 0 <= r <= ny; cell (c, r) spans
 * the vertices (c, r) .. (c + 1, r + 1).  A cell of id a has a boundary edge on every side whose neighbour is off the raster, nodata or not a, directed
 * with a on its right: top (c, r) -> (c + 1, r), right (c + 1, r) -> (c + 1, r + 1), bottom (c + 1, r + 1) -> (c, r + 1), left (c, r + 1) -> (c, r);
 * its key is (r * nx + c) * 4 + side (0 top, 1 right, 2 bottom, 3 left).  The successor of an edge is the boundary edge of the same id that starts where
 * it ends, the one that turns right where there are two, so that 4-connected pieces stay apart.  A ring is a cycle of successors: the vertices at which
 * the direction changes, from its smallest vertex by (r, c), closed by repeating that vertex.  A ring with its interior on the right is an outer ring;
 * a hole of id a that starts at (c0, r0) belongs to the piece of a that holds the cell (c0, r0 - 1).
 * The layer: one feature per id in ascending order; its polygons (one per outer ring) by the start vertex (r, c) of the outer ring; in a polygon the
 * outer ring, then its holes by start vertex.  cells: half the sum of the signed shoelace areas of the feature's rings, which is the number of cells
 * that hold the id.
 *
 * The boundary edges come out of two streaming passes over w on the device (count, then emit at the rank a block scan and a scan of the block totals
 * give: no atomic decides an order, a run gives the same bytes every time), sorted by key, as three columns: key (int64), successor key (int64), id
 * (int32).  The rings are closed on the host by default.  The _gpu_rings entry points close them on the device from the columns where they lie and
 * download only the finished layer; they make the same arrays, and two runs give the same bytes. */
#ifndef TAUDEM_AMD_POLYGONIZE_H
#define TAUDEM_AMD_POLYGONIZE_H

typedef struct tdx_polygons tdx_polygons;
typedef struct tdx_polygonize_edges tdx_polygonize_edges;

/* Edges and rings in one call.  *polygons is the caller's: tdx_polygons_free.  TDX_ERR_NOMEM: the edge columns do not fit; nothing was written. */
int tdx_polygonize_dev(tdx_context* ctx, const int32_t* d_w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats);
int tdx_polygonize(tdx_context* ctx, const int32_t* w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats);
/* Row strips: d_w is an array of ny_local + 2 rows whose row 1 is row row0 of a raster of ny_total rows; the halo rows 0 and ny_local + 1 hold the
 * neighbouring strips' rows and are the CALLER's to fill: the call reads them and never writes them.  A row outside 0 .. ny_total - 1 is off the raster
 * whatever its halo row holds; such a halo row is not read.  The part holds the edges of the owned rows with the keys of the whole raster.
 * Nothing is exchanged: comm is taken like every strip call takes it, and is not used (NULL is fine).  *part is the caller's: tdx_polygonize_edges_free. */
int tdx_polygonize_edges_strip(tdx_context* ctx, const tdx_comm* comm, const int32_t* d_w, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total,
                               int32_t w_nodata, tdx_polygonize_edges** part, tdx_stats* stats);
/* Host code, no context: a part from the caller's columns (n values each, copied). */
int tdx_polygonize_edges_create(const int64_t* keys, const int64_t* next_keys, const int32_t* ids, int64_t n, tdx_polygonize_edges** part);
int64_t tdx_polygonize_edges_count(const tdx_polygonize_edges* part);
/* keys, next_keys, ids: count values each; phase_ms [TDX_POLYGONIZE_PHASES] (any may be NULL) */
void tdx_polygonize_edges_copy(const tdx_polygonize_edges* part, int64_t* keys, int64_t* next_keys, int32_t* ids, double* phase_ms);
void tdx_polygonize_edges_free(tdx_polygonize_edges* part);
/* Host code, no context: the parts of ALL strips in strip order, which is key order -> the polygons of the raster.  TDX_ERR_ARG (with the reason in
 * tdx_last_error(NULL)): keys that do not ascend, a key outside the raster, a successor key that is not among the keys (parts out of order, a strip
 * missing), successors that are no permutation.  The phase times of the parts are carried over (the maximum over the parts). */
int tdx_polygonize_rings(const tdx_polygonize_edges* const* parts, int64_t n_parts, int64_t nx, int64_t ny, tdx_polygons** polygons);

/* Edges and rings on the device: what tdx_polygonize_dev / tdx_polygonize make, array for array, without the edge columns leaving the device or being
 * allocated on the host.  Edge indices are 32-bit there: TDX_ERR_ARG (with a message) for 2^32 - 1 edges or more.  TDX_ERR_NOMEM: the columns or
 * the ring workspace (about 33 bytes per edge and 150 per ring) do not fit; nothing was written. */
int tdx_polygonize_gpu_rings_dev(tdx_context* ctx, const int32_t* d_w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats);
int tdx_polygonize_gpu_rings(tdx_context* ctx, const int32_t* w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats);
/* tdx_polygonize_rings with the rings closed on the device of ctx: the parts are joined, uploaded and closed there.  The same refusals (TDX_ERR_ARG
 * with the same reasons, nothing returned). */
int tdx_polygonize_rings_gpu(tdx_context* ctx, const tdx_polygonize_edges* const* parts, int64_t n_parts, int64_t nx, int64_t ny, tdx_polygons** polygons,
                             tdx_stats* stats);

/* Number of features; *n_polygons, *n_rings, *n_vertices, *n_edges may be NULL. */
int64_t tdx_polygons_count(const tdx_polygons* polygons, int64_t* n_polygons, int64_t* n_rings, int64_t* n_vertices, int64_t* n_edges);
/* ids [features], cells [features], poly_first [features + 1] (the polygons of a feature), ring_first [polygons + 1] (the rings of a polygon: the outer
 * ring first), vert_first [rings + 1], vertices [vertices][2] (column, row), phase_ms [TDX_POLYGONIZE_PHASES]: wall milliseconds of the call's phases,
 * each ended with the stream drained (any may be NULL). */
#define TDX_POLYGONIZE_COUNT 0     /* pass 1 over w: side masks, counts per block */
#define TDX_POLYGONIZE_SCAN 1      /* the scan of the block totals, the read-back of the edge count, the edge columns' allocation */
#define TDX_POLYGONIZE_EMIT 2      /* pass 2 over w: key, successor key and id at every edge's rank */
#define TDX_POLYGONIZE_DOWNLOAD 3  /* the edge columns to the host (device rings: the finished layer to the host) */
#define TDX_POLYGONIZE_RINGS 4     /* the ring builder, on the host (device rings: the sum of its sub-phases) */
#define TDX_POLYGONIZE_PHASES 5
void tdx_polygons_copy(const tdx_polygons* polygons, int32_t* ids, int64_t* cells, int64_t* poly_first, int64_t* ring_first, int64_t* vert_first,
                       int32_t* vertices, double* phase_ms);
/* The device ring builder's sub-phases: ms [TDX_POLYGONIZE_RING_PHASES] wall milliseconds, *rounds the jump rounds of the ring label (at most
 * ceil(log2(edges)) + 1), *workspace_bytes the scratch taken beside the edge columns (any may be NULL).  Returns 1 when the rings of `polygons` were
 * closed on the device, else 0 with everything zero. */
#define TDX_POLYGONIZE_RING_SUCCESSOR 0  /* every successor key to an edge index; the refusals as flags */
#define TDX_POLYGONIZE_RING_VALIDATE 1   /* the successors are a permutation; the flags to the host */
#define TDX_POLYGONIZE_RING_LABEL 2      /* the jump rounds: the ring of every edge and its corner rank; the rings numbered */
#define TDX_POLYGONIZE_RING_PER_RING 3   /* corners, smallest vertex and area of every ring */
#define TDX_POLYGONIZE_RING_RANK 4       /* the rotation to the smallest vertex */
#define TDX_POLYGONIZE_RING_HOLES 5      /* every hole to its outer ring */
#define TDX_POLYGONIZE_RING_ORDER 6      /* the rings sorted, the offset lists, ids and cells */
#define TDX_POLYGONIZE_RING_SCATTER 7    /* every corner to its place */
#define TDX_POLYGONIZE_RING_PHASES 8
int tdx_polygons_ring_phases(const tdx_polygons* polygons, double* ms, int64_t* rounds, int64_t* workspace_bytes);
void tdx_polygons_free(tdx_polygons* polygons);
/* The layer: the fields gridcode (Integer, width 10, 11 where an id of 11 characters occurs: the id) and cells (Integer, width 12); x = gt[0] + c * gt[1], y = gt[3] + r * gt[5] in double (gt: the
 * six numbers of the raster's geotransform).  ESRI shapefile (.shp of shape type 5 with its .shx and .dbf, every ring a part) or GeoJSON (.json /
 * .geojson: Polygon / MultiPolygon, rings reversed as RFC 7946 asks), by the extension of path; any other extension is TDX_ERR_ARG.  No .prj. */
int tdx_polygons_write(const char* path, const tdx_polygons* polygons, const double* gt);

/* Watershed Grid To Shapefile: wfile (read as int32 with its nodata value) -> polyfile.  An extension of polyfile that no writer exists for is
 * refused before anything is read.  With tdx_tool_set_gpus(N) every rank takes the edges of its row strip and the parts are merged on the host. */
int tdx_tool_watershedgridtoshp(const char* wfile, const char* polyfile);
/* Where tdx_tool_watershedgridtoshp closes the rings: 0 on the host (the default), 1 on the device (with N GPUs: the parts merged on rank 0's
 * device).  Any other value is TDX_ERR_ARG and changes nothing. */
int tdx_tool_set_polygon_rings(int where);

#endif /* TAUDEM_AMD_POLYGONIZE_H */
