/* Test infrastructure for tests/golden/make_golden_netlayer.py: every OGR call of src/CatchOutlets.cpp over handles of our own, so that the unmodified
 * reference tool links against oracle/gdal_shim and runs on a stream network layer that exists only as the text record
 * tests/streamnet/ogr_record_lines_stub.h leaves of the reference's StreamNet:
 *   - OGROpen(path) reads that record - one line per feature, "<vertices> <x0> <y0> ... <field name>=<value> ..." - and serves exactly it back through
 *     the read calls the file uses: field index by name, OGR_G_GetPointCount / OGR_G_GetPoint, the integer and double getters (strtol / strtod of the
 *     recorded text, which is %d and %.17g: the values the reference would have handed to a driver, before any driver rounds them);
 *   - the point features it creates are recorded like tests/outlets/ogr_record_stub.h records them, "<x> <y> <field name>=<value> ..." with %.17g, into
 *     `<output path>.rec` - appended feature by feature, because the reference never closes its output data source.
 * Passed with `-include` to CatchOutlets.cpp alone.  The calls the shim declares for its own outlet reader are renamed for that translation unit. */
#ifndef TDX_OGR_REPLAY_LINES_STUB_H
#define TDX_OGR_REPLAY_LINES_STUB_H
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ogr_api.h"

namespace tdx_rep {
struct FieldDefn { std::string name; OGRFieldType type; };
struct Feature;
struct Layer {   /* data source = layer = feature definition */
    std::string path;           /* an output layer: where its record goes */
    std::vector<FieldDefn> fields;
    std::vector<Feature*> features;   /* an input layer */
    size_t next = 0;
};
struct Geometry { std::vector<double> xy; };
struct Feature { Layer* layer; std::vector<std::string> values; Geometry geom; bool owned_by_layer = false; };
static int driver_token;
static inline std::string num(double v) { char b[64]; snprintf(b, sizeof b, "%.17g", v); return b; }
}  // namespace tdx_rep

static inline void tdx_rep_RegisterAll(void) {}
static inline OGRDataSourceH tdx_rep_Open(const char* path, int, OGRSFDriverH*) {
    std::ifstream in(path);
    if (!in) return nullptr;
    tdx_rep::Layer* l = new tdx_rep::Layer;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream is(line);
        size_t np = 0;
        if (!(is >> np)) continue;
        tdx_rep::Feature* f = new tdx_rep::Feature;
        f->layer = l; f->owned_by_layer = true;
        std::string tok;
        for (size_t k = 0; k < 2 * np && (is >> tok); k++) f->geom.xy.push_back(strtod(tok.c_str(), nullptr));
        size_t k = 0;
        while (is >> tok) {
            const size_t eq = tok.find('=');
            const std::string name = tok.substr(0, eq), value = eq == std::string::npos ? std::string() : tok.substr(eq + 1);
            if (l->features.empty()) l->fields.push_back({name, value.find_first_of(".eEn") == std::string::npos ? OFTInteger : OFTReal});
            f->values.push_back(value);
            k++;
        }
        l->features.push_back(f);
    }
    return l;
}
static inline OGRLayerH tdx_rep_DS_GetLayer(OGRDataSourceH ds, int) { return ds; }
static inline GIntBig tdx_rep_L_GetFeatureCount(OGRLayerH l, int) { return GIntBig(static_cast<tdx_rep::Layer*>(l)->features.size()); }
static inline OGRFeatureDefnH tdx_rep_L_GetLayerDefn(OGRLayerH l) { return l; }
static inline int OGR_FD_GetFieldIndex(OGRFeatureDefnH d, const char* name) {
    const tdx_rep::Layer* l = static_cast<tdx_rep::Layer*>(d);
    for (size_t k = 0; k < l->fields.size(); k++) if (l->fields[k].name == name) return int(k);
    return -1;
}
static inline OGRFieldDefnH tdx_rep_FD_GetFieldDefn(OGRFeatureDefnH d, int i) { return &static_cast<tdx_rep::Layer*>(d)->fields[size_t(i)]; }
static inline void tdx_rep_L_ResetReading(OGRLayerH l) { static_cast<tdx_rep::Layer*>(l)->next = 0; }
static inline OGRFeatureH tdx_rep_L_GetNextFeature(OGRLayerH l) {
    tdx_rep::Layer* layer = static_cast<tdx_rep::Layer*>(l);
    return layer->next < layer->features.size() ? layer->features[layer->next++] : nullptr;
}
static inline int tdx_rep_F_GetFieldAsInteger(OGRFeatureH f, int i) { return int(strtol(static_cast<tdx_rep::Feature*>(f)->values[size_t(i)].c_str(), nullptr, 10)); }
static inline double tdx_rep_F_GetFieldAsDouble(OGRFeatureH f, int i) { return strtod(static_cast<tdx_rep::Feature*>(f)->values[size_t(i)].c_str(), nullptr); }
static inline OGRGeometryH tdx_rep_F_GetGeometryRef(OGRFeatureH f) { return &static_cast<tdx_rep::Feature*>(f)->geom; }
static inline int OGR_G_GetPointCount(OGRGeometryH g) { return int(static_cast<tdx_rep::Geometry*>(g)->xy.size() / 2); }
static inline void OGR_G_GetPoint(OGRGeometryH g, int i, double* x, double* y, double* z) {
    const tdx_rep::Geometry* ge = static_cast<tdx_rep::Geometry*>(g);
    *x = ge->xy[size_t(2 * i)]; *y = ge->xy[size_t(2 * i + 1)]; *z = 0.0;
}

static inline OGRSFDriverH OGRGetDriverByName(const char*) { return &tdx_rep::driver_token; }
static inline void CSLDestroy(char**) {}
static inline OGRDataSourceH OGR_Dr_CreateDataSource(OGRSFDriverH, const char* path, char**) {
    tdx_rep::Layer* l = new tdx_rep::Layer;
    l->path = std::string(path) + ".rec";
    if (FILE* f = fopen(l->path.c_str(), "w")) fclose(f);   /* a run that writes no outlet leaves an empty record */
    return l;
}
static inline OGRLayerH OGR_DS_CreateLayer(OGRDataSourceH ds, const char*, OGRSpatialReferenceH, OGRwkbGeometryType, char**) { return ds; }
static inline OGRFieldDefnH OGR_Fld_Create(const char* name, OGRFieldType type) { return new tdx_rep::FieldDefn{name, type}; }
static inline void OGR_Fld_SetWidth(OGRFieldDefnH, int) {}
static inline int OGR_L_CreateField(OGRLayerH l, OGRFieldDefnH f, int) { static_cast<tdx_rep::Layer*>(l)->fields.push_back(*static_cast<tdx_rep::FieldDefn*>(f)); return 0; }
static inline OGRFeatureH OGR_F_Create(OGRFeatureDefnH d) {
    tdx_rep::Feature* f = new tdx_rep::Feature;
    f->layer = static_cast<tdx_rep::Layer*>(d);
    f->values.resize(f->layer->fields.size());
    return f;
}
static inline void OGR_F_SetFieldInteger(OGRFeatureH f, int i, int v) { static_cast<tdx_rep::Feature*>(f)->values[size_t(i)] = std::to_string(v); }
static inline void OGR_F_SetFieldDouble(OGRFeatureH f, int i, double v) { static_cast<tdx_rep::Feature*>(f)->values[size_t(i)] = tdx_rep::num(v); }
static inline OGRGeometryH OGR_G_CreateGeometry(OGRwkbGeometryType) { return new tdx_rep::Geometry; }
static inline void OGR_G_SetPoint_2D(OGRGeometryH g, int, double x, double y) { static_cast<tdx_rep::Geometry*>(g)->xy = {x, y}; }
static inline int OGR_F_SetGeometry(OGRFeatureH f, OGRGeometryH g) { static_cast<tdx_rep::Feature*>(f)->geom = *static_cast<tdx_rep::Geometry*>(g); return 0; }
static inline void OGR_G_DestroyGeometry(OGRGeometryH g) { delete static_cast<tdx_rep::Geometry*>(g); }
static inline int OGR_L_CreateFeature(OGRLayerH l, OGRFeatureH f) {
    const tdx_rep::Layer* layer = static_cast<tdx_rep::Layer*>(l);
    const tdx_rep::Feature* ft = static_cast<tdx_rep::Feature*>(f);
    std::string line = tdx_rep::num(ft->geom.xy.at(0)) + " " + tdx_rep::num(ft->geom.xy.at(1));
    for (size_t k = 0; k < layer->fields.size(); k++) line += " " + layer->fields[k].name + "=" + ft->values[k];
    if (FILE* fp = fopen(layer->path.c_str(), "a")) { fprintf(fp, "%s\n", line.c_str()); fclose(fp); }
    return 0;
}
static inline void tdx_rep_F_Destroy(OGRFeatureH f) { if (f && !static_cast<tdx_rep::Feature*>(f)->owned_by_layer) delete static_cast<tdx_rep::Feature*>(f); }
static inline void tdx_rep_DS_Destroy(OGRDataSourceH) {}

#define OGRRegisterAll tdx_rep_RegisterAll
#define OGROpen tdx_rep_Open
#define OGR_DS_GetLayer tdx_rep_DS_GetLayer
#define OGR_L_GetFeatureCount tdx_rep_L_GetFeatureCount
#define OGR_L_GetLayerDefn tdx_rep_L_GetLayerDefn
#define OGR_FD_GetFieldDefn tdx_rep_FD_GetFieldDefn
#define OGR_L_ResetReading tdx_rep_L_ResetReading
#define OGR_L_GetNextFeature tdx_rep_L_GetNextFeature
#define OGR_F_GetFieldAsInteger tdx_rep_F_GetFieldAsInteger
#define OGR_F_GetFieldAsDouble tdx_rep_F_GetFieldAsDouble
#define OGR_F_GetGeometryRef tdx_rep_F_GetGeometryRef
#define OGR_F_Destroy tdx_rep_F_Destroy
#define OGR_DS_Destroy tdx_rep_DS_Destroy
#endif
