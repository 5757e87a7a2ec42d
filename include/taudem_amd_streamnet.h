/* taudem_amd_streamnet.h - the StreamNet part of the C ABI of libtaudem_amd.so.  Included by taudem_amd.h (inside its extern "C" block, after the
 * types tdx_context, tdx_comm and tdx_stats): include that header, not this one. */
#ifndef TAUDEM_AMD_STREAMNET_H
#define TAUDEM_AMD_STREAMNET_H

/* StreamNet: netsetup() src/streamnet.cpp:372-1508 on one rank, whose link numbers are the only fixed target (they come from one counter in the
 * order the reference's queues pop, so its own output changes with its rank count).  From p (int16), src (int32; a stream cell has src not nodata,
 * src > 0 and p not nodata), fel and ad8 (float32, read without a nodata test) it makes
 *   ord    int16: the Strahler order on the stream cells, 0 everywhere else (the file's nodata value is -32768, no cell holds it);
 *   w      int32: the id of the link that drains the cell - the catchment grid CatchHydroGeo and InunDepth take - MISSINGLONG (-2147483647) where
 *          no stream is reached; with single_watershed (-sw) 1 on every reached cell and on every stream cell;
 *   links  the rows of the -tree file (9 int64 per link: link, first and last row of its points in coord, downstream link, the two upstream
 *          links, order, outlet id, magnitude) and of the -coord file (5 doubles per point: x, y, distance to the outlet along the stream,
 *          elevation, contributing area = ad8 * dxA * dyA as a float), in the reference's order.
 * dxc / dyc: the cell sizes of every row (host); dxA / dyA: those of the middle row (tiffIO's); gt: {x of the left edge, cell width, y of the top
 * edge, cell height} of the raster file (host, 4 doubles).  Outlets: HOST column / row / id lists in file order (outlet_id NULL: 1, 2, ...); an
 * outlet on a stream cell ends a link there, the last one on a cell wins, outlets off the raster or off the stream change nothing.
 * The two dense passes (the distance to the outlet along the stream, the catchment labels) and the compaction of the stream cells run on the
 * device; the link numbering walks the stream cells alone, on the host.  *links is owned by the caller: tdx_streamnet_links_free.
 * tdx_streamnet_gpu_links / tdx_streamnet_gpu_links_dev: the same arguments and the same results, byte for byte, with the links built on the device too
 * (the queue's pop order has a closed form): the compact columns, the labels and the orders never leave the device, only the tree and coord rows come
 * down into the handle, which everything below takes unchanged.  They take fewer than 2^31 - 1 stream cells (TDX_ERR_ARG beyond).  The level pass of
 * the device builder takes as many rounds as there are links on the longest path of the network. */
typedef struct tdx_streamnet_links tdx_streamnet_links;
int tdx_streamnet_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx, int64_t ny,
                      int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt,
                      const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* d_ord,
                      int32_t* d_w, tdx_streamnet_links** links, tdx_stats* stats);
int tdx_streamnet(tdx_context* ctx, const int16_t* p, const int32_t* src, const float* fel, const float* ad8, int64_t nx, int64_t ny, int16_t p_nodata,
                  int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
                  const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* ord, int32_t* w,
                  tdx_streamnet_links** links, tdx_stats* stats);
int tdx_streamnet_gpu_links_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx, int64_t ny,
                                int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt,
                                const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed,
                                int16_t* d_ord, int32_t* d_w, tdx_streamnet_links** links, tdx_stats* stats);
int tdx_streamnet_gpu_links(tdx_context* ctx, const int16_t* p, const int32_t* src, const float* fel, const float* ad8, int64_t nx, int64_t ny, int16_t p_nodata,
                            int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
                            const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* ord, int32_t* w,
                            tdx_streamnet_links** links, tdx_stats* stats);
/* Number of links; *n_points: rows of coord; *stream_cells: cells on the stream (either may be NULL). */
int64_t tdx_streamnet_links_count(const tdx_streamnet_links* links, int64_t* n_points, int64_t* stream_cells);
/* tree [links][9], coord [points][5], phase_ms [TDX_STREAMNET_PHASES]: wall milliseconds of the call's phases, each ended with the stream drained
 * (any may be NULL). */
#define TDX_STREAMNET_SETUP 0    /* info words and steps of the length sweep */
#define TDX_STREAMNET_LENGTH 1   /* the length sweep */
#define TDX_STREAMNET_COMPACT 2  /* compaction of the stream cells and their copy to the host */
#define TDX_STREAMNET_LINKS 3    /* the link builder, whichever ran (host: the walk; device: its launches and the download of the rows) */
#define TDX_STREAMNET_SCATTER 4  /* info words of the label sweep, labels and orders of the stream cells */
#define TDX_STREAMNET_LABEL 5    /* the label sweep */
#define TDX_STREAMNET_TOTAL 6    /* the sum of the six */
#define TDX_STREAMNET_PHASES 7
void tdx_streamnet_links_copy(const tdx_streamnet_links* links, int64_t* tree, double* coord, double* phase_ms);
void tdx_streamnet_links_free(tdx_streamnet_links* links);
/* The device builder's own record: 1 and the values when the links of the handle were built on the device, 0 (nothing written) otherwise.  ms
 * [TDX_STREAMNET_DLINK_PHASES]: wall milliseconds of its sub-phases, each ended with the stream drained; the pointer-jumping rounds along the cells with
 * one inflow; the rounds of the level pass over the link tree; the scratch bytes taken beside the columns, the coord rows included.  Any may be NULL. */
#define TDX_STREAMNET_DLINK_CLASSIFY 0   /* outlets onto the cells, inflow table, classes, node numbers */
#define TDX_STREAMNET_DLINK_JUMP 1       /* pointer jumping along the cells with one inflow */
#define TDX_STREAMNET_DLINK_LEVEL 2      /* order, magnitude, h and root by levels over the link tree */
#define TDX_STREAMNET_DLINK_NUMBER 3     /* the sort by (h, root) and the scan: link numbers */
#define TDX_STREAMNET_DLINK_LINKS 4      /* the link table, labels and orders of the stream cells */
#define TDX_STREAMNET_DLINK_ROWS 5       /* the tree rows and the coord rows */
#define TDX_STREAMNET_DLINK_DOWNLOAD 6   /* tree and coord to the host */
#define TDX_STREAMNET_DLINK_PHASES 7
int tdx_streamnet_links_device_phases(const tdx_streamnet_links* links, double* ms, int64_t* jump_rounds, int64_t* level_rounds, int64_t* workspace_bytes);
/* Row strips (arrays of ny_local + 2 rows; dxc / dyc of those rows; row0: the global row of the strip's first owned row).  The work is cut where the
 * data has to meet: every strip compacts the stream cells of its OWNED rows, the caller puts the parts together in strip order - that is the row-major
 * order of the whole raster - and builds the links once, and every strip gets its share of the labels back.  The result is byte for byte the
 * one-device result for any cut.
 *   tdx_streamnet_compact_strip   exchanges the halo rows of p and src (it writes them), runs the length sweep on the strip and returns the strip's part.
 *   tdx_streamnet_links_build     host code, no context: the parts of ALL strips in strip order (handles of this process) -> the links of the raster;
 *                                 outlets as for tdx_streamnet, with GLOBAL rows.
 *   tdx_streamnet_links_build_gpu the same on the device of ctx: the parts are put together on the host, uploaded in strip order, and the links built
 *                                 there; the labels and orders come down into the handle with the rows (a few bytes per stream cell), so that
 *                                 tdx_streamnet_label_strip takes the handle unchanged on whichever context labels the strip.
 *   tdx_streamnet_label_strip     the strip's labels and orders (first_cell: the number of stream cells in the strips above it), the label sweep on the
 *                                 strip; d_ord / d_w of ny_local + 2 rows, the owned rows are the result.  p / src must still hold their halo rows. */
typedef struct tdx_streamnet_compact tdx_streamnet_compact;
int tdx_streamnet_compact_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx,
                                int64_t ny_local, int64_t row0, int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc,
                                tdx_streamnet_compact** part, tdx_stats* stats);
int64_t tdx_streamnet_compact_count(const tdx_streamnet_compact* part);
void tdx_streamnet_compact_free(tdx_streamnet_compact* part);
int tdx_streamnet_links_build(const tdx_streamnet_compact* const* parts, int64_t n_parts, int64_t nx, int64_t ny, double dxA, double dyA, const double* gt,
                              const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, tdx_streamnet_links** links);
int tdx_streamnet_links_build_gpu(tdx_context* ctx, const tdx_streamnet_compact* const* parts, int64_t n_parts, int64_t nx, int64_t ny, double dxA, double dyA,
                                  const double* gt, const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets,
                                  tdx_streamnet_links** links);
int tdx_streamnet_label_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny_local, int16_t p_nodata,
                              int32_t src_nodata, const tdx_streamnet_compact* part, const tdx_streamnet_links* links, int64_t first_cell,
                              int single_watershed, int16_t* d_ord, int32_t* d_w, tdx_stats* stats);
/* The -tree and / or the -coord file from the rows (src/streamnet.cpp:1165, :1177; either name may be NULL: that file is not touched).  Returns 0 or
 * TDX_ERR_FILE. */
int tdx_streamnet_write_text(const tdx_streamnet_links* links, const char* treefile, const char* coordfile);
/* The stream network layer (-net) from the link rows: reachshape() src/streamnet.cpp:244-365 per link, in tree order.  Host code, no context, no GPU.
 *   tdx_streamnet_net_rows   tree [n_links][9] and coord [n_points][5] as tdx_streamnet_links_copy returns them (columns 2..4 of coord hold float values and
 *                            are used as floats: the reference's arithmetic on them is float arithmetic) -> real [n_links][9]: Length, DSContArea, strmDrop,
 *                            Slope, StraightL, USContArea, DOUTEND, DOUTSTART, DOUTMID; first [n_links + 1]: offsets into x / y; x, y [n_vertices]: the
 *                            vertices of every link REVERSED, so that vertex 0 is its downstream end (a link of one point is a line of ONE vertex, as the
 *                            reference writes it).  n_vertices: the sum over the links of tree[.][2] - tree[.][1] + 1.  geographic: the raster's flag -
 *                            every segment then goes through tiffIO::geotoLength (src/tiffIO.cpp:434), which needs nothing else of the raster.
 *                            TDX_ERR_ARG: a link's rows lie outside coord, or n_vertices is not that sum.
 *   tdx_streamnet_net_write  the layer of those lines with the reference's 17 fields (LINKNO, DSLINKNO, USLINKNO1, USLINKNO2: width 6; DSNODEID: 12;
 *                            strmOrder: 6; Length: 16.1; Magnitude: 6; DSContArea: 16.1; strmDrop: 16.2; Slope: 16.12; StraightL: 16.1; USContArea:
 *                            16.1; WSNO: 6; DOUTEND, DOUTSTART, DOUTMID: 16.1) as an ESRI shapefile or GeoJSON, by the extension of path.  Returns 0,
 *                            TDX_ERR_ARG (extension) or TDX_ERR_FILE. */
int tdx_streamnet_net_rows(const int64_t* tree, const double* coord, int64_t n_links, int64_t n_points, int geographic, int64_t n_vertices, double* real,
                           int64_t* first, double* x, double* y);
int tdx_streamnet_net_write(const tdx_streamnet_links* links, int geographic, const char* path);
/* int netsetup(char* pfile, char* srcfile, char* ordfile, char* ad8file, char* elevfile, char* treefile, char* coordfile, char* outletsds,
 *              char* lyrname, int uselayername, int lyrno, char* wfile, char* streamnetsrc, char* streamnetlyr, long useOutlets, long ordert,
 *              bool verbose)                                                                                            src/streamnet.cpp:372
 * ordert = 0 is -sw.  The -net layer is not written: a call with a non-empty streamnetsrc or streamnetlyr is refused before anything is read
 * (tdx_streamnet_net_write makes the layer from the links of tdx_streamnet). */
int tdx_tool_streamnet(const char* pfile, const char* srcfile, const char* ordfile, const char* ad8file, const char* elevfile, const char* treefile,
                       const char* coordfile, const char* outletsds, const char* lyrname, int uselayername, int lyrno, const char* wfile,
                       const char* streamnetsrc, const char* streamnetlyr, long useOutlets, long ordert, int verbose);
/* Where tdx_tool_streamnet builds the links from now on: 0 the host (the default), 1 the device - with --gpus N rank 0 builds them on its device.  Both
 * write the same bytes.  TDX_ERR_ARG for any other value. */
int tdx_tool_set_streamnet_links(int where);

#endif /* TAUDEM_AMD_STREAMNET_H */
