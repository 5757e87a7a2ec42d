// Point and line layers: the writer the outlet tools share, the reader of ALL fields of an outlet source (read_outlets of outlets.hpp returns x, y and an
// id and stays as it is), and the line layer StreamNet's network is written as and CatchOutlets reads.  Host code without HIP headers.  Replaces the OGR
// calls of src/MoveOutletsToStrm.cpp:214-279, :812-886, src/ConnectDown.cpp:649-861, src/streamnet.cpp:107-365 and src/CatchOutlets.cpp:131-260.
//   ESRI shapefile  .shp + .shx + .dbf, shape type Point or PolyLine (one part per feature), Integer / Real / String fields.  Widths are the reference's
//                   where it sets them (Dist_moved: 6; the 17 fields of the stream network) and otherwise what OGR's shapefile driver is believed to
//                   default to: Integer 9 (widened to the longest value), Real 24 with 15 decimals, String 80.  No .prj: the GeoTIFF reader keeps no WKT.
//   GeoJSON         .json / .geojson, a FeatureCollection of Point or LineString features with properties; coordinates and Real values with 17
//                   significant digits.
// The watershed polygons (polygonize.hip) are a third geometry, written only: shape type Polygon with every ring a part, GeoJSON Polygon / MultiPolygon.
// Any other extension is refused (layer_kind() == LayerKind::None) before a tool reads anything.
// Carry-over: a field read from a .dbf keeps its 32-byte descriptor and the bytes of every record, so that .dbf -> .dbf is byte-faithful per column;
// across formats N / F with 0 decimals is Integer, N / F with decimals Real, anything else String.
// A line of a single vertex is legal in both directions and both formats: the reference's StreamNet writes such lines for links of one cell.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace tdx {
enum class LayerKind { None, Shapefile, GeoJSON };
enum class FieldType { Integer, Real, String };
struct LayerField {
    std::string name;
    FieldType type = FieldType::Integer;
    int width = 0, decimals = 0;   // 0 width: the default of the type
    std::string dbf_descriptor;     // 32 bytes when the field came out of a .dbf: its values are the records' bytes, `width` of them each
};
// The attribute table of a layer: what point and line layers share
struct LayerTable {
    std::vector<LayerField> fields;
    std::vector<std::vector<std::string>> values;   // [feature][field]: text; "" is a null
    size_t add_field(const std::string& name, FieldType type, int width = 0, int decimals = 0);   // returns its index; every feature gets a null
    int field_index(const std::string& name) const;   // -1: no such field
    void set(size_t feature, size_t field, long long v);
    void set(size_t feature, size_t field, double v);
    void set(size_t feature, size_t field, const std::string& v) { values[feature][field] = v; }
};
struct PointLayer : LayerTable {
    std::vector<double> x, y;
    void resize(size_t n);   // n features
};
struct LineLayer : LayerTable {
    std::vector<std::vector<double>> x, y;   // [feature][vertex]
    void resize(size_t n);   // n features, without vertices
};

// features -> polygons -> rings -> vertices.  A ring repeats its first vertex at its end; the outer ring of a polygon comes first and runs clockwise
// (the shapefile convention), its holes follow and run counter-clockwise.
struct PolygonLayer : LayerTable {
    struct Ring { std::vector<double> x, y; };
    typedef std::vector<Ring> Polygon;
    std::vector<std::vector<Polygon>> polygons;   // [feature][polygon][ring]
    void resize(size_t n);   // n features, without polygons
};

LayerKind layer_kind(const std::string& path);
extern const char* const kLayerKindsMessage;   // names the two supported kinds
extern const char* const kLineLayerKindsMessage;
extern const char* const kPolygonLayerKindsMessage;
// All fields of an outlet source, one row per feature that read_outlets() returns for the same file (n_features of them, else an error): the
// descriptors and records of the .dbf next to a .shp, the properties of GeoJSON Point features, the id column of a text file (an Integer field "id").
bool read_point_fields(const std::string& path, size_t n_features, PointLayer& layer, std::string& err);
bool write_point_layer(const std::string& path, const PointLayer& layer, std::string& err);
// Shapefile: shape type 3 (PolyLine), one part per feature.  GeoJSON: LineString features.
bool write_line_layer(const std::string& path, const LineLayer& layer, std::string& err);
// Shapefile: shape types 3, 13 and 23 (Z and M are ignored, of several parts the first is taken, a null shape is a line without vertices) with the .dbf
// next to it.  GeoJSON: the LineString features in document order (of a MultiLineString the first part) with their properties.
bool read_line_layer(const std::string& path, LineLayer& layer, std::string& err);
// Shapefile: shape type 5 (Polygon), every ring of a feature a part, in the layer's order.  GeoJSON: a Polygon for a feature of one polygon, else a
// MultiPolygon; every ring is written REVERSED (RFC 7946: exterior rings counter-clockwise, holes clockwise), from and to the same start vertex.  A layer
// without features is a valid empty file.
bool write_polygon_layer(const std::string& path, const PolygonLayer& layer, std::string& err);
// Shapefile: shape types 5, 15 and 25 (Z and M are ignored, a null shape is a feature without rings) with the .dbf next to it.  GeoJSON: the Polygon
// and MultiPolygon features in document order with their properties.  Every part / ring becomes the one ring of a polygon of its own: nesting is not
// rebuilt (an even-odd fill does not need it).  Files whose headers, record lengths, counts, part indices or .dbf record counts lie are refused.
bool read_polygon_layer(const std::string& path, PolygonLayer& layer, std::string& err);
// the files write_point_layer(path) / write_line_layer(path) / write_polygon_layer(path) create
std::vector<std::string> layer_files(const std::string& path);
}  // namespace tdx
