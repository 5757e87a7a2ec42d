/* taudem_amd_catchoutlets.h - line layers and CatchOutlets in the C ABI of libtaudem_amd.so.  All of it is host code: no function here takes a context or
 * touches a GPU.  Included by taudem_amd.h (inside its extern "C" block): include that header, not this one. */
#ifndef TAUDEM_AMD_CATCHOUTLETS_H
#define TAUDEM_AMD_CATCHOUTLETS_H

/* A line layer: ESRI shapefile (.shp of shape type 3, PolyLine, one part per feature, with its .shx and .dbf) or GeoJSON (.json / .geojson, LineString
 * features), chosen by the extension of path; any other extension is TDX_ERR_ARG.  Feature i has the vertices first[i] .. first[i + 1] - 1 of x / y
 * (first: n + 1 offsets); a feature of one vertex is legal.  types[k]: 0 Integer (columns[k]: int32_t*), 1 Real (double*), 2 String (const char* const*).
 * widths / decimals (nfields each, both or neither; 0 = the type's default, as tdx_points_write uses) size the columns of the .dbf.  No .prj is written. */
int tdx_lines_write(const char* path, const int64_t* first, const double* x, const double* y, int64_t n, int32_t nfields, const char* const* names,
                    const int32_t* types, const int32_t* widths, const int32_t* decimals, const void* const* columns);
/* Reads one: shapefile shape types 3, 13 and 23 (Z and M ignored, the first part of several, a null shape is a feature without vertices) with the fields of
 * its .dbf, or the LineString features of a GeoJSON file with their properties.  *layer is the caller's: tdx_line_layer_free. */
typedef struct tdx_line_layer tdx_line_layer;
int tdx_lines_read(const char* path, tdx_line_layer** layer);
/* features; *n_vertices, *n_fields may be NULL */
int64_t tdx_line_layer_count(const tdx_line_layer* layer, int64_t* n_vertices, int32_t* n_fields);
/* first: features + 1 offsets; x, y: all vertices (any may be NULL) */
void tdx_line_layer_vertices(const tdx_line_layer* layer, int64_t* first, double* x, double* y);
/* the name of field k (NULL: no such field); *type 0 Integer, 1 Real, 2 String; *width, *decimals: of a .dbf column, else 0 */
const char* tdx_line_layer_field(const tdx_line_layer* layer, int32_t k, int32_t* type, int32_t* width, int32_t* decimals);
/* the text of field k of a feature: the bytes of the .dbf cell, or the JSON number / string; "" is a null.  Valid until the layer is freed. */
const char* tdx_line_layer_value(const tdx_line_layer* layer, int64_t feature, int32_t k);
void tdx_line_layer_free(tdx_line_layer* layer);

/* CatchOutlets on a link table (src/CatchOutlets.cpp:280-368, :87-121).  Row i: the link's numbers, DOUTEND, DOUTSTART, USContArea and its downstream and
 * upstream end.  Links with dslinkno < 0 or an upstream link are kept.  For every kept link with dslinkno < 0, in table order: its downstream end is
 * mapped to a cell of pfile (tiffIO::geoToGlobalXY, truncation towards zero); off the raster, or with p outside 1..8 there, nothing is written and nothing
 * walked; else the centre of the cell one step down p (of the cell itself where that step leaves the raster) is written with DOUTEND = the link's DOUTEND
 * and Id = the counter, which starts at gwstartno, and uslinkno1's subtree is visited before uslinkno2's with downout = 0.  Visiting a link: not kept -
 * stop; DOUTSTART - downout > mindist and USContArea > minarea - its upstream end is written with DOUTEND = its DOUTSTART (the reference's choice) and
 * the next Id, and downout = DOUTSTART from here up this path; its upstream links are visited only if USContArea > minarea.
 * Of pfile the header and one cell per outlet link are read.  The walk keeps its own stack (no recursion); a cycle of upstream links is TDX_ERR_ARG.
 * out_*: room for `capacity` outlets (2 * n_links holds every tree); *n_out: how many were written.  out_row: the link's row in the table.
 * TDX_ERR_FILE: pfile or one of its cells cannot be read.  TDX_ERR_ARG: also when capacity does not hold the outlets. */
int tdx_catchoutlets(const char* pfile, const int32_t* linkno, const int32_t* dslinkno, const int32_t* uslinkno1, const int32_t* uslinkno2, const double* doutend,
                     const double* doutstart, const double* uscontarea, const double* down_x, const double* down_y, const double* up_x, const double* up_y,
                     int64_t n_links, double mindist, int32_t gwstartno, double minarea, int64_t capacity, int64_t* out_row, double* out_x, double* out_y,
                     double* out_doutend, int32_t* out_id, int64_t* n_out);

/* int catchoutlets(char *pfile, char *streamnetsrc, char *outletsdatasrc, double mindist, int gwstartno, double minarea)      src/CatchOutlets.cpp:126
 * The network comes from ONE of: streamnetsrc, a line layer with the fields LINKNO, DSLINKNO, USLINKNO1, USLINKNO2, DOUTEND, DOUTSTART, USContArea (the
 * layer tdx_streamnet_net_write makes, or the CPU TauDEM's) - a missing field is named and refused; or treefile and coordfile, this project's streamnet
 * -tree and -coord outputs.  Both or neither (an empty string counts as not given, NULL too) is TDX_ERR_ARG, as is an extension of streamnetsrc or
 * outletsdatasrc that no reader or writer exists for: all before anything is read.  The outlets are written as a point layer with the fields LINKNO,
 * DSLINKNO, USLINKNO1, USLINKNO2 (Integer 6), DOUTEND (Real 16.1), Id (Integer 10). */
int tdx_tool_catchoutlets(const char* pfile, const char* streamnetsrc, const char* treefile, const char* coordfile, const char* outletsdatasrc, double mindist,
                          int gwstartno, double minarea);

#endif /* TAUDEM_AMD_CATCHOUTLETS_H */
