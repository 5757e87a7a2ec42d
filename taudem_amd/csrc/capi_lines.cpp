// The host-only part of the C ABI: line layers (include/taudem_amd_catchoutlets.h), the stream network layer from the link rows
// (tdx_streamnet_net_rows / _write, include/taudem_amd_streamnet.h) and CatchOutlets on a link table.  No function here creates a context or calls HIP.
#include <cstring>
#include <string>
#include <vector>

#include "catchoutlets.hpp"
#include "context.hpp"
#include "geotiff.hpp"
#include "streamnet_net.hpp"
#include "vector_layer.hpp"

struct tdx_line_layer {
    tdx::LineLayer layer;
};

extern "C" {

int tdx_lines_write(const char* path, const int64_t* first, const double* x, const double* y, int64_t n, int32_t nfields, const char* const* names,
                    const int32_t* types, const int32_t* widths, const int32_t* decimals, const void* const* columns) {
    if (!path || n < 0 || nfields < 0 || (n > 0 && !first) || (nfields > 0 && (!names || !types || !columns)) || (widths == nullptr) != (decimals == nullptr))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_lines_write: bad argument");
    if (tdx::layer_kind(path) == tdx::LayerKind::None) return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_lines_write: unsupported output ") + path + ": " + tdx::kLineLayerKindsMessage);
    tdx::LineLayer L;
    for (int32_t k = 0; k < nfields; k++) {
        if (!names[k] || types[k] < 0 || types[k] > 2 || (n > 0 && !columns[k]) || (widths && (widths[k] < 0 || widths[k] > 254 || decimals[k] < 0 || decimals[k] > widths[k])))
            return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_lines_write: bad argument");
        L.add_field(names[k], types[k] == 0 ? tdx::FieldType::Integer : types[k] == 1 ? tdx::FieldType::Real : tdx::FieldType::String, widths ? widths[k] : 0, widths ? decimals[k] : 0);
    }
    L.resize(size_t(n));
    for (int64_t i = 0; i < n; i++) {
        if (first[i] < 0 || first[i + 1] < first[i] || (first[i + 1] > first[i] && (!x || !y))) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_lines_write: bad argument");
        L.x[size_t(i)].assign(x + first[i], x + first[i + 1]);
        L.y[size_t(i)].assign(y + first[i], y + first[i + 1]);
        for (int32_t k = 0; k < nfields; k++) {
            if (types[k] == 0) L.set(size_t(i), size_t(k), (long long)static_cast<const int32_t*>(columns[k])[i]);
            else if (types[k] == 1) L.set(size_t(i), size_t(k), static_cast<const double*>(columns[k])[i]);
            else { const char* s = static_cast<const char* const*>(columns[k])[i]; L.set(size_t(i), size_t(k), std::string(s ? s : "")); }
        }
    }
    std::string err;
    if (!tdx::write_line_layer(path, L, err)) return tdx_fail(nullptr, TDX_ERR_FILE, err);
    return TDX_OK;
}

int tdx_lines_read(const char* path, tdx_line_layer** layer) {
    if (!path || !layer) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_lines_read: bad argument");
    *layer = nullptr;
    if (tdx::layer_kind(path) == tdx::LayerKind::None) return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_lines_read: unsupported input ") + path + ": " + tdx::kLineLayerKindsMessage);
    tdx_line_layer* h = new tdx_line_layer;
    std::string err;
    if (!tdx::read_line_layer(path, h->layer, err)) { delete h; return tdx_fail(nullptr, TDX_ERR_FILE, err); }
    *layer = h;
    return TDX_OK;
}

int64_t tdx_line_layer_count(const tdx_line_layer* h, int64_t* n_vertices, int32_t* n_fields) {
    if (n_vertices) *n_vertices = 0;
    if (n_fields) *n_fields = 0;
    if (!h) return 0;
    if (n_vertices) for (const auto& v : h->layer.x) *n_vertices += int64_t(v.size());
    if (n_fields) *n_fields = int32_t(h->layer.fields.size());
    return int64_t(h->layer.x.size());
}

void tdx_line_layer_vertices(const tdx_line_layer* h, int64_t* first, double* x, double* y) {
    if (!h) return;
    int64_t at = 0;
    for (size_t i = 0; i < h->layer.x.size(); i++) {
        if (first) first[i] = at;
        for (size_t k = 0; k < h->layer.x[i].size(); k++, at++) {
            if (x) x[at] = h->layer.x[i][k];
            if (y) y[at] = h->layer.y[i][k];
        }
    }
    if (first) first[h->layer.x.size()] = at;
}

const char* tdx_line_layer_field(const tdx_line_layer* h, int32_t k, int32_t* type, int32_t* width, int32_t* decimals) {
    if (!h || k < 0 || size_t(k) >= h->layer.fields.size()) return nullptr;
    const tdx::LayerField& f = h->layer.fields[size_t(k)];
    if (type) *type = f.type == tdx::FieldType::Integer ? 0 : f.type == tdx::FieldType::Real ? 1 : 2;
    if (width) *width = f.width;
    if (decimals) *decimals = f.decimals;
    return f.name.c_str();
}

const char* tdx_line_layer_value(const tdx_line_layer* h, int64_t feature, int32_t k) {
    if (!h || feature < 0 || size_t(feature) >= h->layer.values.size() || k < 0 || size_t(k) >= h->layer.values[size_t(feature)].size()) return nullptr;
    return h->layer.values[size_t(feature)][size_t(k)].c_str();
}

void tdx_line_layer_free(tdx_line_layer* h) { delete h; }

int tdx_streamnet_net_rows(const int64_t* tree, const double* coord, int64_t n_links, int64_t n_points, int geographic, int64_t n_vertices, double* real,
                           int64_t* first, double* x, double* y) {
    if (n_links < 0 || n_points < 0 || n_vertices < 0 || (n_links > 0 && (!tree || !coord || !real || !first)) || (n_vertices > 0 && (!x || !y)))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_net_rows: bad argument");
    streamnet::NetRows rows;
    std::string err;
    if (!streamnet::net_rows(tree, coord, n_links, n_points, geographic != 0, rows, err)) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_net_rows: " + err);
    if (int64_t(rows.x.size()) != n_vertices)
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_net_rows: the links have " + std::to_string(rows.x.size()) + " vertices, not " + std::to_string(n_vertices));
    if (n_links > 0) {
        memcpy(real, rows.real.data(), rows.real.size() * sizeof(double));
        memcpy(first, rows.first.data(), rows.first.size() * sizeof(int64_t));
    }
    if (n_vertices > 0) {
        memcpy(x, rows.x.data(), rows.x.size() * sizeof(double));
        memcpy(y, rows.y.data(), rows.y.size() * sizeof(double));
    }
    return TDX_OK;
}

int tdx_streamnet_net_write(const tdx_streamnet_links* links, int geographic, const char* path) {
    if (!links || !path) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_net_write: bad argument");
    if (tdx::layer_kind(path) == tdx::LayerKind::None)
        return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_streamnet_net_write: unsupported output ") + path + ": " + tdx::kLineLayerKindsMessage);
    int64_t n_points = 0;
    const int64_t n_links = tdx_streamnet_links_count(links, &n_points, nullptr);
    std::vector<int64_t> tree(size_t(n_links) * 9);
    std::vector<double> coord(size_t(n_points) * 5);
    tdx_streamnet_links_copy(links, tree.data(), coord.data(), nullptr);
    streamnet::NetRows rows;
    std::string err;
    if (!streamnet::net_rows(tree.data(), coord.data(), n_links, n_points, geographic != 0, rows, err)) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_net_write: " + err);
    tdx::LineLayer L;
    streamnet::net_layer(tree.data(), n_links, rows, L);
    if (!tdx::write_line_layer(path, L, err)) return tdx_fail(nullptr, TDX_ERR_FILE, err);
    return TDX_OK;
}

int tdx_catchoutlets(const char* pfile, const int32_t* linkno, const int32_t* dslinkno, const int32_t* uslinkno1, const int32_t* uslinkno2, const double* doutend,
                     const double* doutstart, const double* uscontarea, const double* down_x, const double* down_y, const double* up_x, const double* up_y,
                     int64_t n_links, double mindist, int32_t gwstartno, double minarea, int64_t capacity, int64_t* out_row, double* out_x, double* out_y,
                     double* out_doutend, int32_t* out_id, int64_t* n_out) {
    if (!pfile || n_links < 0 || capacity < 0 || !n_out ||
        (n_links > 0 && (!linkno || !dslinkno || !uslinkno1 || !uslinkno2 || !doutend || !doutstart || !uscontarea || !down_x || !down_y || !up_x || !up_y)) ||
        (capacity > 0 && (!out_row || !out_x || !out_y || !out_doutend || !out_id)))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_catchoutlets: bad argument");
    *n_out = 0;
    tdx::TiffReader rd;
    if (!rd.open(pfile)) return tdx_fail(nullptr, TDX_ERR_FILE, "tdx_catchoutlets: " + rd.error());
    const tdx::RasterInfo ri = rd.info();
    tdx::FlowGrid g;
    g.nx = ri.nx; g.ny = ri.ny; g.xleftedge = ri.xleftedge; g.ytopedge = ri.ytopedge; g.dlon = ri.dlon; g.dlat = ri.dlat;
    g.p_at = [&](int64_t col, int64_t row, int16_t& d) { return rd.read_window(col, row, 1, 1, tdx::DType::I16, &d); };
    std::vector<tdx::NetLink> links(static_cast<size_t>(n_links));
    for (int64_t i = 0; i < n_links; i++)
        links[size_t(i)] = {linkno[i], dslinkno[i], uslinkno1[i], uslinkno2[i], doutend[i], doutstart[i], uscontarea[i], down_x[i], down_y[i], up_x[i], up_y[i]};
    std::vector<tdx::CatchOutlet> out;
    std::string err;
    if (!tdx::catch_outlets(links, g, mindist, gwstartno, minarea, out, err)) {
        const bool io = err.rfind("cannot read", 0) == 0;
        return tdx_fail(nullptr, io ? TDX_ERR_FILE : TDX_ERR_ARG, "tdx_catchoutlets: " + err + (io ? ": " + rd.error() : ""));
    }
    if (int64_t(out.size()) > capacity) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_catchoutlets: " + std::to_string(out.size()) + " outlets, room for " + std::to_string(capacity));
    for (size_t i = 0; i < out.size(); i++) { out_row[i] = out[i].row; out_x[i] = out[i].x; out_y[i] = out[i].y; out_doutend[i] = out[i].doutend; out_id[i] = out[i].id; }
    *n_out = int64_t(out.size());
    return TDX_OK;
}

}  // extern "C"
