/* Test infrastructure for tests/golden/make_golden_outlets.py: the OGR *write* calls of src/MoveOutletsToStrm.cpp and src/ConnectDown.cpp over
 * handles of our own that RECORD every created feature, so that the unmodified reference tools link against oracle/gdal_shim, run to their end and
 * leave what they would have written as text: on OGR_DS_Destroy the data source `path` becomes the file `path.rec`, one line per feature in the
 * order of creation:
 *     <x %.17g> <y %.17g> <field name>=<value> ...        (Integer %d, Real %.17g, String as it is; a field never set has an empty value)
 * Passed with `-include` to those two translation units alone.  The outlet READER stays the shim's: the four calls that both sides use
 * (OGR_DS_Destroy, OGR_L_GetLayerDefn, OGR_F_GetFieldIndex, OGR_F_Destroy) are renamed for the translation unit and go to the shim for a handle that
 * is not ours.  The shim's layer has one Integer field, the id: a field definition that is not ours is recorded as "id". */
#ifndef TDX_OGR_RECORD_STUB_H
#define TDX_OGR_RECORD_STUB_H
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "ogr_api.h"

#define OGRERR_NONE 0

namespace tdx_rec {
struct FieldDefn { std::string name; OGRFieldType type; };
struct Layer { std::string path; std::vector<FieldDefn> fields; std::vector<std::string> lines; };   /* data source = layer = feature definition */
struct Feature { Layer* layer; std::vector<std::string> values; double x = 0, y = 0; };
struct Geometry { double x = 0, y = 0; };
static inline std::set<void*>& ours() { static std::set<void*> s; return s; }
static inline bool is_ours(void* h) { return h && ours().count(h) != 0; }
template <class T> static inline T* make() { T* t = new T; ours().insert(t); return t; }
static int driver_token;
static inline std::string num(double v) { char b[64]; snprintf(b, sizeof b, "%.17g", v); return b; }
}  // namespace tdx_rec

static inline OGRSFDriverH OGRGetDriverByName(const char*) { return &tdx_rec::driver_token; }
static inline int OGRGetDriverCount(void) { return 0; }
static inline OGRSFDriverH OGRGetDriver(int) { return &tdx_rec::driver_token; }
static inline const char* OGR_Dr_GetName(OGRSFDriverH) { return "record"; }
static inline void OGRCleanupAll(void) {}
static inline void GDALDestroyDriverManager(void) {}
static inline void CSLDestroy(char**) {}
static inline OGRDataSourceH OGR_Dr_CreateDataSource(OGRSFDriverH, const char* path, char**) {
    tdx_rec::Layer* l = tdx_rec::make<tdx_rec::Layer>();
    l->path = path;
    return l;
}
static inline OGRLayerH OGR_DS_CreateLayer(OGRDataSourceH ds, const char*, OGRSpatialReferenceH, OGRwkbGeometryType, char**) { return ds; }
static inline OGRFieldDefnH OGR_Fld_Create(const char* name, OGRFieldType type) {
    tdx_rec::FieldDefn* f = tdx_rec::make<tdx_rec::FieldDefn>();
    f->name = name; f->type = type;
    return f;
}
static inline void OGR_Fld_SetWidth(OGRFieldDefnH, int) {}
static inline int OGR_L_CreateField(OGRLayerH l, OGRFieldDefnH f, int) {
    tdx_rec::Layer* layer = static_cast<tdx_rec::Layer*>(l);
    if (tdx_rec::is_ours(f)) layer->fields.push_back(*static_cast<tdx_rec::FieldDefn*>(f));
    else layer->fields.push_back(tdx_rec::FieldDefn{"id", OFTInteger});
    return 0;
}
static inline OGRFeatureH OGR_F_Create(OGRFeatureDefnH d) {
    tdx_rec::Feature* f = tdx_rec::make<tdx_rec::Feature>();
    f->layer = static_cast<tdx_rec::Layer*>(d);
    f->values.resize(f->layer->fields.size());
    return f;
}
static inline void tdx_rec_set(OGRFeatureH f, int i, const std::string& v) {
    tdx_rec::Feature* ft = static_cast<tdx_rec::Feature*>(f);
    if (i >= 0 && size_t(i) < ft->values.size()) ft->values[size_t(i)] = v;
}
static inline void OGR_F_SetFieldInteger(OGRFeatureH f, int i, int v) { tdx_rec_set(f, i, std::to_string(v)); }
static inline void OGR_F_SetFieldDouble(OGRFeatureH f, int i, double v) { tdx_rec_set(f, i, tdx_rec::num(v)); }
static inline void OGR_F_SetFieldString(OGRFeatureH f, int i, const char* v) { tdx_rec_set(f, i, v ? v : ""); }
static inline OGRGeometryH OGR_G_CreateGeometry(OGRwkbGeometryType) { return tdx_rec::make<tdx_rec::Geometry>(); }
static inline void OGR_G_SetPoint_2D(OGRGeometryH g, int, double x, double y) { static_cast<tdx_rec::Geometry*>(g)->x = x; static_cast<tdx_rec::Geometry*>(g)->y = y; }
static inline int OGR_F_SetGeometry(OGRFeatureH f, OGRGeometryH g) {
    static_cast<tdx_rec::Feature*>(f)->x = static_cast<tdx_rec::Geometry*>(g)->x;
    static_cast<tdx_rec::Feature*>(f)->y = static_cast<tdx_rec::Geometry*>(g)->y;
    return 0;
}
static inline void OGR_G_DestroyGeometry(OGRGeometryH g) { tdx_rec::ours().erase(g); delete static_cast<tdx_rec::Geometry*>(g); }
static inline int OGR_L_CreateFeature(OGRLayerH l, OGRFeatureH f) {
    tdx_rec::Layer* layer = static_cast<tdx_rec::Layer*>(l);
    const tdx_rec::Feature* ft = static_cast<tdx_rec::Feature*>(f);
    std::string line = tdx_rec::num(ft->x) + " " + tdx_rec::num(ft->y);
    for (size_t k = 0; k < layer->fields.size(); k++) line += " " + layer->fields[k].name + "=" + (k < ft->values.size() ? ft->values[k] : std::string());
    layer->lines.push_back(line);
    return OGRERR_NONE;
}
static inline int OGR_FD_GetFieldCount(OGRFeatureDefnH d) { return tdx_rec::is_ours(d) ? int(static_cast<tdx_rec::Layer*>(d)->fields.size()) : 1; }

/* the four calls both sides use */
static inline void tdx_rec_DS_Destroy(OGRDataSourceH ds) {
    if (!tdx_rec::is_ours(ds)) { if (ds) OGR_DS_Destroy(ds); return; }
    tdx_rec::Layer* l = static_cast<tdx_rec::Layer*>(ds);
    if (FILE* f = fopen((l->path + ".rec").c_str(), "w")) {
        for (const std::string& s : l->lines) fprintf(f, "%s\n", s.c_str());
        fclose(f);
    }
    tdx_rec::ours().erase(ds);
    delete l;
}
static inline OGRFeatureDefnH tdx_rec_L_GetLayerDefn(OGRLayerH l) { return tdx_rec::is_ours(l) ? l : OGR_L_GetLayerDefn(l); }
static inline int tdx_rec_F_GetFieldIndex(OGRFeatureH f, const char* name) {
    if (!tdx_rec::is_ours(f)) return OGR_F_GetFieldIndex(f, name);
    const tdx_rec::Layer* l = static_cast<tdx_rec::Feature*>(f)->layer;
    for (size_t k = 0; k < l->fields.size(); k++) if (l->fields[k].name == name) return int(k);
    return -1;
}
static inline void tdx_rec_F_Destroy(OGRFeatureH f) {
    if (!tdx_rec::is_ours(f)) { OGR_F_Destroy(f); return; }
    tdx_rec::ours().erase(f);
    delete static_cast<tdx_rec::Feature*>(f);
}
#define OGR_DS_Destroy tdx_rec_DS_Destroy
#define OGR_L_GetLayerDefn tdx_rec_L_GetLayerDefn
#define OGR_F_GetFieldIndex tdx_rec_F_GetFieldIndex
#define OGR_F_Destroy tdx_rec_F_Destroy
#endif
