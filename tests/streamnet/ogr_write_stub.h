/* Test infrastructure for tests/golden/make_golden_streamnet.py: the OGR *write* calls of src/streamnet.cpp (createStreamNetShapefile,
 * reachshape) as no-ops over fake handles, so that the unmodified reference tool links against oracle/gdal_shim and runs to its end without
 * writing the -net layer (which no golden holds).  Passed with `-include` to streamnet.cpp alone.  OGR_L_GetLayerDefn, OGR_F_GetFieldIndex and
 * OGR_DS_Destroy are renamed for that one translation unit: the shim's versions expect handles of its own outlet reader. */
#ifndef TDX_OGR_WRITE_STUB_H
#define TDX_OGR_WRITE_STUB_H
#include "ogr_api.h"

namespace tdx_ogr_stub {
static int token;
static inline void* handle() { return &token; }
}  // namespace tdx_ogr_stub

static inline OGRSFDriverH OGRGetDriverByName(const char*) { return tdx_ogr_stub::handle(); }
static inline OGRDataSourceH OGR_Dr_CreateDataSource(OGRSFDriverH, const char*, char**) { return tdx_ogr_stub::handle(); }
static inline OGRLayerH OGR_DS_CreateLayer(OGRDataSourceH, const char*, OGRSpatialReferenceH, OGRwkbGeometryType, char**) { return tdx_ogr_stub::handle(); }
static inline void CSLDestroy(char**) {}
static inline OGRFieldDefnH OGR_Fld_Create(const char*, OGRFieldType) { return tdx_ogr_stub::handle(); }
static inline void OGR_Fld_SetWidth(OGRFieldDefnH, int) {}
static inline void OGR_Fld_SetPrecision(OGRFieldDefnH, int) {}
static inline int OGR_L_CreateField(OGRLayerH, OGRFieldDefnH, int) { return 0; }
static inline OGRFeatureH OGR_F_Create(OGRFeatureDefnH) { return tdx_ogr_stub::handle(); }
static inline void OGR_F_SetFieldInteger(OGRFeatureH, int, int) {}
static inline void OGR_F_SetFieldDouble(OGRFeatureH, int, double) {}
static inline OGRGeometryH OGR_G_CreateGeometry(OGRwkbGeometryType) { return tdx_ogr_stub::handle(); }
static inline void OGR_G_AddPoint(OGRGeometryH, double, double, double) {}
static inline int OGR_F_SetGeometryDirectly(OGRFeatureH, OGRGeometryH) { return 0; }
static inline int OGR_L_CreateFeature(OGRLayerH, OGRFeatureH) { return 0; }

static inline OGRFeatureDefnH tdx_stub_L_GetLayerDefn(OGRLayerH) { return tdx_ogr_stub::handle(); }
static inline int tdx_stub_F_GetFieldIndex(OGRFeatureH, const char*) { return 0; }
static inline void tdx_stub_DS_Destroy(OGRDataSourceH) {}
#define OGR_L_GetLayerDefn tdx_stub_L_GetLayerDefn
#define OGR_F_GetFieldIndex tdx_stub_F_GetFieldIndex
#define OGR_DS_Destroy tdx_stub_DS_Destroy
#endif
