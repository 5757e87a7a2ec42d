/* Test infrastructure for tests/golden/make_golden_netlayer.py: the OGR *write* calls of src/streamnet.cpp (createStreamNetShapefile, reachshape) over
 * handles of our own that RECORD every created line feature, so that the unmodified reference tool links against oracle/gdal_shim, runs to its end and
 * leaves its -net layer as text: on OGR_DS_Destroy the data source `path` becomes the file `path.rec`, one line per feature in the order of creation:
 *     <vertices> <x0> <y0> <x1> <y1> ... <field name>=<value> ...        (coordinates and Real values %.17g, Integer %d)
 * Passed with `-include` to streamnet.cpp alone (tests/streamnet/ogr_write_stub.h, which records nothing, stays what make_golden_streamnet.py uses).
 * OGR_L_GetLayerDefn, OGR_F_GetFieldIndex and OGR_DS_Destroy are renamed for that one translation unit: the shim's versions expect handles of its own
 * outlet reader. */
#ifndef TDX_OGR_RECORD_LINES_STUB_H
#define TDX_OGR_RECORD_LINES_STUB_H
#include <cstdio>
#include <string>
#include <vector>

#include "ogr_api.h"

namespace tdx_lrec {
struct FieldDefn { std::string name; OGRFieldType type; };
struct Layer { std::string path; std::vector<FieldDefn> fields; std::vector<std::string> lines; };   /* data source = layer = feature definition */
struct Geometry { std::vector<double> xy; };
struct Feature { Layer* layer; std::vector<std::string> values; Geometry* geom = nullptr; };
static int driver_token;
static inline std::string num(double v) { char b[64]; snprintf(b, sizeof b, "%.17g", v); return b; }
}  // namespace tdx_lrec

static inline OGRSFDriverH OGRGetDriverByName(const char*) { return &tdx_lrec::driver_token; }
static inline OGRDataSourceH OGR_Dr_CreateDataSource(OGRSFDriverH, const char* path, char**) {
    tdx_lrec::Layer* l = new tdx_lrec::Layer;
    l->path = path;
    return l;
}
static inline OGRLayerH OGR_DS_CreateLayer(OGRDataSourceH ds, const char*, OGRSpatialReferenceH, OGRwkbGeometryType, char**) { return ds; }
static inline void CSLDestroy(char**) {}
static inline OGRFieldDefnH OGR_Fld_Create(const char* name, OGRFieldType type) { return new tdx_lrec::FieldDefn{name, type}; }
static inline void OGR_Fld_SetWidth(OGRFieldDefnH, int) {}
static inline void OGR_Fld_SetPrecision(OGRFieldDefnH, int) {}
static inline int OGR_L_CreateField(OGRLayerH l, OGRFieldDefnH f, int) {
    static_cast<tdx_lrec::Layer*>(l)->fields.push_back(*static_cast<tdx_lrec::FieldDefn*>(f));
    return 0;
}
static inline OGRFeatureH OGR_F_Create(OGRFeatureDefnH d) {
    tdx_lrec::Feature* f = new tdx_lrec::Feature;
    f->layer = static_cast<tdx_lrec::Layer*>(d);
    f->values.resize(f->layer->fields.size());
    return f;
}
static inline void tdx_lrec_set(OGRFeatureH f, int i, const std::string& v) {
    tdx_lrec::Feature* ft = static_cast<tdx_lrec::Feature*>(f);
    if (i >= 0 && size_t(i) < ft->values.size()) ft->values[size_t(i)] = v;
}
static inline void OGR_F_SetFieldInteger(OGRFeatureH f, int i, int v) { tdx_lrec_set(f, i, std::to_string(v)); }
static inline void OGR_F_SetFieldDouble(OGRFeatureH f, int i, double v) { tdx_lrec_set(f, i, tdx_lrec::num(v)); }
static inline OGRGeometryH OGR_G_CreateGeometry(OGRwkbGeometryType) { return new tdx_lrec::Geometry; }
static inline void OGR_G_AddPoint(OGRGeometryH g, double x, double y, double) {
    static_cast<tdx_lrec::Geometry*>(g)->xy.push_back(x);
    static_cast<tdx_lrec::Geometry*>(g)->xy.push_back(y);
}
static inline int OGR_F_SetGeometryDirectly(OGRFeatureH f, OGRGeometryH g) { static_cast<tdx_lrec::Feature*>(f)->geom = static_cast<tdx_lrec::Geometry*>(g); return 0; }
static inline int OGR_L_CreateFeature(OGRLayerH l, OGRFeatureH f) {
    tdx_lrec::Layer* layer = static_cast<tdx_lrec::Layer*>(l);
    const tdx_lrec::Feature* ft = static_cast<tdx_lrec::Feature*>(f);
    const std::vector<double> none;
    const std::vector<double>& xy = ft->geom ? ft->geom->xy : none;
    std::string line = std::to_string(xy.size() / 2);
    for (double v : xy) line += " " + tdx_lrec::num(v);
    for (size_t k = 0; k < layer->fields.size(); k++) line += " " + layer->fields[k].name + "=" + ft->values[k];
    layer->lines.push_back(line);
    return 0;
}

static inline OGRFeatureDefnH tdx_lrec_L_GetLayerDefn(OGRLayerH l) { return l; }
static inline int tdx_lrec_F_GetFieldIndex(OGRFeatureH f, const char* name) {
    const tdx_lrec::Layer* l = static_cast<tdx_lrec::Feature*>(f)->layer;
    for (size_t k = 0; k < l->fields.size(); k++) if (l->fields[k].name == name) return int(k);
    return -1;
}
static inline void tdx_lrec_DS_Destroy(OGRDataSourceH ds) {
    tdx_lrec::Layer* l = static_cast<tdx_lrec::Layer*>(ds);
    if (!l) return;
    if (FILE* f = fopen((l->path + ".rec").c_str(), "w")) {
        for (const std::string& s : l->lines) fprintf(f, "%s\n", s.c_str());
        fclose(f);
    }
    delete l;
}
#define OGR_L_GetLayerDefn tdx_lrec_L_GetLayerDefn
#define OGR_F_GetFieldIndex tdx_lrec_F_GetFieldIndex
#define OGR_DS_Destroy tdx_lrec_DS_Destroy
#endif
