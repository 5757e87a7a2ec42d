// File-level tool functions: same argument lists, banners, timing blocks and error codes as the
// reference's tool functions, with the compute part on the GPU.  `tool --gpus N` / TAUDEM_AMD_GPUS=N / tdx_tool_set_gpus(N)
// partitions the raster into N row strips, one GPU (and one host thread) each, exchanging boundary rows over RCCL
// (tool_strips.hpp, comm.cpp) - the place of `mpiexec -n N` in the reference.
//
// Every tool function runs on one frame, ToolRun: banner, input() per raster (compared with the first one, under the tool's mismatch
// policy), outlets(), read_done(), compute(one GPU: tdx_x() on a context of its own; N GPUs: tdx_x_strip() on strip arrays),
// output() per raster, finish(footer).  A tool function states what is its own: which rasters as which type and in which order,
// the two library calls, which header and nodata value each output carries, and the footer's wording.
//   tdx_tool_pitremove           <- flood()               src/flood.cpp:50-526
//   tdx_tool_d8flowdir           <- setdird8()            src/d8.cpp:181-355
//   tdx_tool_dinfflowdir         <- setdir()              src/dinf.cpp:109-284
//   tdx_tool_aread8              <- aread8()              src/aread8.cpp:56-322
//   tdx_tool_areadinf            <- area()                src/areadinf.cpp:53-300
//   tdx_tool_dinfdecayaccum      <- dmarea()              src/dinfdecayaccum.cpp:61-324
//   tdx_tool_gridnet             <- gridnet()             src/gridnet.cpp:54-510
//   tdx_tool_d8flowpathextremeup <- d8flowpathextremeup() src/D8flowpathextremeup.cpp:58-285
//   tdx_tool_threshold           <- threshold()           src/Threshold.cpp:49-161
//   tdx_tool_dinfupdependence    <- depgrd()              src/DinfUpDependence.cpp:52-272
//   tdx_tool_dinfrevaccum        <- dsaccum()             src/DinfRevAccum.cpp:51-290
//   tdx_tool_dinfconclimaccum    <- dsllArea()            src/DinfConcLimAccum.cpp:61-326
//   tdx_tool_dinftranslimaccum   <- tlaccum()             src/DinfTransLimAccum.cpp:61-372
//   tdx_tool_dinfdistdown        <- dinfdistdown()        src/DinfDistDown.cpp:66-1060
//   tdx_tool_dinfdistup          <- dinfdistup()          src/DinfDistUp.cpp:65-1214
//   tdx_tool_retlimflow          <- retlimro()            src/RetlimFlow.cpp:53-240
//   tdx_tool_dinfavalanche       <- avalancherunoutgrd()  src/DinfAvalanche.cpp:62-420
//   tdx_tool_d8hdisttostrm       <- distgrid()            src/D8HDistToStrm.cpp:57-260
//   tdx_tool_gagewatershed       <- gagewatershed()       src/gagewatershed.cpp:56-360
//   tdx_tool_flowdircond         <- flowdircond()         src/flowdircond.cpp:54-252
//   tdx_tool_d8vdisttostrm       <- d8vdistdown()         src/D8VDistToStrm.cpp:58-276
//   tdx_tool_slopeavedown        <- sloped()              src/SlopeAveDown.cpp:59-330
//   tdx_tool_catchhydrogeo       <- catchhydrogeo()       src/CatchHydroGeo.cpp:69-413
//   tdx_tool_inundepth           <- inundepth()           src/InunDepth.cpp:53-545
//   tdx_tool_dropanalysis        <- dropan()              src/DropAnalysis.cpp:172-705
//   tdx_tool_peukerdouglas       <- peukerdouglas()       src/PeukerDouglas.cpp:54-241
//   tdx_tool_sinmapsi            <- sindexcombined()      src/SinmapSI.cpp:138-441
//   tdx_tool_twi                 <- twigrid()             src/TWI.cpp:49-153
//   tdx_tool_slopearea           <- slopearea()           src/SlopeArea.cpp:52-152
//   tdx_tool_slopearearatio      <- atanbgrid()           src/SlopeAreaRatio.cpp:49-148
//   tdx_tool_lengtharea          <- lengtharea()          src/LengthArea.cpp:51-149
//   tdx_tool_setregion           <- setregion()           src/SetRegion.cpp:78-191
//   tdx_tool_editraster          <- editraster()          src/EditRaster.cpp:69-168
//   tdx_tool_catchoutlets        <- catchoutlets()        src/CatchOutlets.cpp:126-443   (host code: no GPU)
//   tdx_tool_moveoutletstostrm   <- outletstosrc()        src/MoveOutletsToStrm.cpp:80-914
//   tdx_tool_connectdown         <- connectdown()         src/ConnectDown.cpp:79-893
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "context.hpp"
#include "catchoutlets.hpp"
#include "dropan_table.hpp"
#include "editraster_changes.hpp"
#include "geotiff.hpp"
#include "hand_tables.hpp"
#include "outlets.hpp"
#include "sinmap_table.hpp"
#include "tool_strips.hpp"
#include "vector_layer.hpp"
#include "region_table.hpp"
#include <sys/stat.h>

#define TDVERSION "5.4.0"   /* src/commonLib.h:63 */

namespace {

using toolstrips::Outlets;
using toolstrips::RankJob;

int g_tool_device = -1;
int g_tool_gpus = -1;
int g_tool_streamnet_links = 0;   // tdx_tool_set_streamnet_links: 0 the host builds the links of streamnet, 1 the device
int g_tool_polygon_rings = 0;   // tdx_tool_set_polygon_rings: 0 the host closes the rings of watershedgridtoshp, 1 the device

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int tool_device() {
    if (g_tool_device >= 0) return g_tool_device;
    const char* e = getenv("TAUDEM_AMD_DEVICE");
    return e ? atoi(e) : 0;
}
int tool_gpus() {
    int n = g_tool_gpus;
    if (n < 1) { const char* e = getenv("TAUDEM_AMD_GPUS"); n = e ? atoi(e) : 1; }
    return n < 1 ? 1 : n;
}
void report(tdx_context* c) { fprintf(stderr, "taudem_amd: %s\n", tdx_last_error(c)); }
bool want_lzw() {
    const char* e = getenv("TAUDEM_AMD_COMPRESS");
    if (e && (strcmp(e, "NONE") == 0 || strcmp(e, "none") == 0)) return false;
    return true;   // the reference writes COMPRESS=LZW (src/tiffIO.cpp:316-318)
}

struct Raster {
    std::string path;
    tdx::RasterInfo info;
    std::vector<float> f;
    std::vector<int16_t> s;
    std::vector<int32_t> l;
};

// tiffIO constructor + CreateNewPartition prints + read (src/tiffIO.cpp:54-183, src/createpart.h:49-87)
// Reads rows [y0, y1) of an open raster into the full-size host array `base`.
static bool read_rows(tdx::TiffReader& rd, tdx::DType type, void* base, int64_t nx, int64_t y0, int64_t y1) {
    return rd.read_window(0, y0, nx, y1 - y0, type, static_cast<char*>(base) + size_t(y0) * size_t(nx) * tdx::dtype_size(type));
}

int load_raster(const char* path, tdx::DType type, Raster& r) {
    tdx::TiffReader rd;
    if (!rd.open(path)) {
        printf("Error opening file %s.\n", path);
        fflush(stdout);
        g_tdx_thread_error = rd.error();
        return TDX_ERR_FILE;
    }
    r.info = rd.info();
    if (!r.info.geographic) printf("Input file %s has projected coordinate system.\n", path);
    else printf("Input file %s has geographic coordinate system.\n", path);
    const size_t n = size_t(r.info.nx) * size_t(r.info.ny);
    printf("Nodata value input to create partition from file: %lf\n", r.info.nodata);
    void* base;
    if (type == tdx::DType::F32) {
        printf("Nodata value recast to float used in partition raster: %f\n", (float)r.info.nodata);
        r.f.resize(n);
        base = r.f.data();
    } else if (type == tdx::DType::I32) {
        printf("Nodata value recast to int32_t used in partition raster: %d\n", (int32_t)r.info.nodata);
        r.l.resize(n);
        base = r.l.data();
    } else {
        printf("Nodata value recast to int16_t used in partition raster: %d\n", (int16_t)r.info.nodata);
        r.s.resize(n);
        base = r.s.data();
    }
    fflush(stdout);
    // With --gpus N every rank reads its OWN rows - the strip partition of the compute (src/linearpart.h:133-134), each through its own
    // reader on the file, like the ranks of the reference (src/tiffIO.cpp:186-290) - instead of one thread decoding a 17 GB raster.
    const int nrd = int(std::min<int64_t>(std::min(tool_gpus(), 64), r.info.ny));
    bool ok = true;
    std::string err;
    if (nrd <= 1) {
        ok = read_rows(rd, type, base, r.info.nx, 0, r.info.ny);
        if (!ok) err = rd.error();
    } else {
        rd.close();
        std::vector<std::thread> th;
        std::vector<std::string> errs(static_cast<size_t>(nrd));
        const int64_t rows = r.info.ny / nrd;
        for (int k = 0; k < nrd; k++)
            th.emplace_back([&, k] {
                tdx::TiffReader mine;
                const int64_t y0 = int64_t(k) * rows, y1 = (k == nrd - 1) ? r.info.ny : int64_t(k + 1) * rows;
                if (!mine.open(path) || !read_rows(mine, type, base, r.info.nx, y0, y1)) errs[size_t(k)] = mine.error().empty() ? "read failed" : mine.error();
            });
        for (auto& t : th) t.join();
        for (const std::string& e : errs) if (!e.empty()) { ok = false; err = e; break; }
    }
    if (!ok) { printf("Error opening file %s.\n", path); g_tdx_thread_error = err; return TDX_ERR_FILE; }
    return TDX_OK;
}

// tiffIO::compareTiff (src/tiffIO.cpp:449-541)
bool compare_rasters(const tdx::RasterInfo& a, const char* an, const tdx::RasterInfo& b, const char* bn) {
    const double tol = 0.0001;
    if (a.nx != b.nx) { printf("Columns do not match: %d %d\n", int(a.nx), int(b.nx)); return false; }
    if (a.ny != b.ny) { printf("Rows do not match: %d %d\n", int(a.ny), int(b.ny)); return false; }
    if (std::fabs(a.dxA() - b.dxA()) > tol) { printf("dx does not match: %lf %lf\n", a.dxA(), b.dxA()); return false; }
    if (std::fabs(a.dyA() - b.dyA()) > tol) { printf("dy does not match: %lf %lf\n", a.dyA(), b.dyA()); return false; }
    if (std::fabs(a.xleftedge - b.xleftedge) > 0.0) {
        printf("Warning! Left edge does not match exactly:\n %lf in file %s\n %lf in file %s\n", a.xleftedge, an, b.xleftedge, bn);
    }
    if (std::fabs(a.ytopedge - b.ytopedge) > 0.0) {
        printf("Warning! Top edge does not match exactly:\n %lf in file %s\n %lf in file %s\n", a.ytopedge, an, b.ytopedge, bn);
    }
    return true;
}

int save_raster(const char* path, tdx::DType type, const void* data, const tdx::RasterInfo& like, double nodata) {
    std::string name = path;
    if (tdx::resolve_output_name(name) != 0) { printf("GDAL driver is not available\n"); fflush(stdout); return TDX_ERR_DRIVER; }
    const size_t cb = tdx::dtype_size(type);
    const double fileGB = double(cb) * double(like.nx) * double(like.ny) / 1000000000.0;
    if (fileGB > 4.0) printf("Setting BIGTIFF, File: %s, Anticipated size (GB):%.2f\n", name.c_str(), fileGB);
    tdx::TiffWriter wr;
    if (!wr.create(name, like.nx, like.ny, type, nodata, &like, want_lzw())) { printf("Error opening file %s.\n", name.c_str()); g_tdx_thread_error = wr.error(); return TDX_ERR_FILE; }
    // with --gpus N the rows are encoded / written by N host threads (each rank's rows, src/tiffIO.cpp:382-427); same bytes for any N
    if (!wr.write_all(data, std::min(tool_gpus(), 64))) { g_tdx_thread_error = wr.error(); return TDX_ERR_FILE; }
    if (!wr.close()) { g_tdx_thread_error = wr.error(); return TDX_ERR_FILE; }
    return TDX_OK;
}

struct CtxGuard {
    tdx_context* c = nullptr;
    int rc;
    CtxGuard() { rc = tdx_context_create(tool_device(), &c); if (rc != TDX_OK) fprintf(stderr, "taudem_amd: %s\n", tdx_last_error(nullptr)); }
    ~CtxGuard() { tdx_context_destroy(c); }
};

// outlets: readoutlets + geoToGlobalXY (src/aread8.cpp:114-136,179-189)
int load_outlets(const char* datasrc, const tdx::RasterInfo& ri, Outlets& o) {
    std::vector<double> x, y; std::vector<int> id; std::string err;
    if (!tdx::read_outlets(datasrc, x, y, id, err)) {
        printf("Error Opening OGR Data Source .\n");
        printf("Error opening shapefile. Exiting \n");
        fflush(stdout);
        g_tdx_thread_error = err;
        return TDX_ERR_OUTLETS;
    }
    printf("Warning: Spatial References of Outlet feature and Raster data are missing.\n");
    o.x.resize(x.size()); o.y.resize(x.size());
    for (size_t i = 0; i < x.size(); i++) {
        int gx, gy;
        tdx::geo_to_global_xy(x[i], y[i], ri.xleftedge, ri.ytopedge, ri.dlon, ri.dlat, gx, gy);
        o.x[i] = gx; o.y[i] = gy;
    }
    o.ids.assign(id.begin(), id.end());
    return TDX_OK;
}

void print_gpu_stats(const char* tool, const tdx_stats& st, int64_t cells) {
    if (!getenv("TAUDEM_AMD_STATS")) return;
    fprintf(stderr, "{\"tool\": \"%s\", \"cells\": %lld, \"device_ms\": %.3f, \"mcells_per_s\": %.3f, \"rounds\": %lld, \"flats\": %lld, "
                    "\"levels_fall\": %lld, \"levels_rise\": %lld}\n",
            tool, (long long)cells, st.ms_total, st.ms_total > 0 ? double(cells) / st.ms_total / 1000.0 : 0.0, (long long)st.rounds,
            (long long)st.flats_initial, (long long)st.levels_fall, (long long)st.levels_rise);
}

// What a tool does with a raster that does not match its first one (tiffIO::compareTiff returned false)
enum class Mismatch {
    Sizes,       // "File sizes do not match" + the file + MPI_Abort(MCW, 5): most tools (e.g. src/gridnet.cpp:147-152)
    Silent,      // return 1 without a word (src/Threshold.cpp:90, src/DinfUpDependence.cpp:103, src/areadinf.cpp:134)
    PitRemove,   // flood()'s own sentence, return 1
    Avalanche    // both file names, return 1: the MPI_Abort is commented out in the reference (src/DinfAvalanche.cpp)
};

// The timing blocks the reference's tools end with
enum class Footer {
    Times,         // <label>: N + read / compute / write / total
    HeaderTimes,   // PitRemove: a header read time of its own (src/flood.cpp:517-519)
    FlowDir,       // D8FlowDir / DinfFlowDir: slopes and flats apart, the slope raster written in between (src/d8.cpp, src/dinf.cpp)
    CountOnly,     // RetLimFlow: the reference prints no times; the count that ran, as the other tools say it
    ComputeOnly,   // CatchHydroGeo / InunDepth: one line, <label>: the whole run in seconds
    NoWrite,       // DropAnalysis: <label>: N + read / compute / total (src/DropAnalysis.cpp:690-692)
    ComputeWrite,  // SinmapSI: "Compute time" from the start of the call (reading included) and "File write time" (src/SinmapSI.cpp:409-435)
    ComputeLine    // TWI, SlopeArea, SlopeAreaRatio, LengthArea: one line, <label>: the compute step alone (src/TWI.cpp:91,132-141)
};

template <class T> constexpr tdx::DType dtype_of();
template <> constexpr tdx::DType dtype_of<float>() { return tdx::DType::F32; }
template <> constexpr tdx::DType dtype_of<int16_t>() { return tdx::DType::I16; }
template <> constexpr tdx::DType dtype_of<int32_t>() { return tdx::DType::I32; }

// One call of a tool function: banner, read, compute, write, footer.  A step that fails leaves its code in `rc`, and every later
// input() / outlets() / output() does nothing, so that a tool checks once per phase: read_done(), compute(), finish().
struct ToolRun {
    double begint, readt = 0, computet = 0;
    const Raster* grid = nullptr;   // the first raster read: every other one is compared with it, and it gives the strips their rows
    int nproc = 1;                  // GPUs (row strips) of the compute step: the count that is printed is the count that ran
    tdx_stats st{};
    int rc = TDX_OK;
    std::optional<CtxGuard> ctx;    // the one-GPU context: it lives until the tool function returns, after the footer's times are taken

    explicit ToolRun(const std::string& name) {
        printf("%s version %s\n", name.c_str(), TDVERSION);
        fflush(stdout);
        begint = now_s();
    }
    size_t cells() const { return size_t(grid->info.nx) * size_t(grid->info.ny); }

    void input(const char* path, tdx::DType type, Raster& r, Mismatch policy = Mismatch::Sizes) {
        if (rc != TDX_OK) return;
        r.path = path;
        rc = load_raster(path, type, r);
        if (rc != TDX_OK) return;
        if (!grid) { grid = &r; return; }
        if (compare_rasters(grid->info, grid->path.c_str(), r.info, path)) return;
        switch (policy) {
        case Mismatch::Sizes: printf("File sizes do not match\n%s\n", path); rc = TDX_ERR_OUTLETS; break;
        case Mismatch::Silent: rc = TDX_ERR_MISMATCH; break;
        case Mismatch::PitRemove:
            printf("Error: depression mask and input DEM are not similar. Files must have the same number of rows/columns.\n");
            rc = TDX_ERR_MISMATCH;
            break;
        case Mismatch::Avalanche: printf("File sizes do not match\n%s\n%s\n", path, grid->path.c_str()); rc = 1; break;
        }
        fflush(stdout);
    }
    // use == 1: read the outlet file; the library is given outlets whenever use is not 0
    void outlets(const char* datasrc, int use, Outlets& o) {
        if (rc != TDX_OK) return;
        o.use = use != 0;
        if (use == 1) rc = load_outlets(datasrc, grid->info, o);
    }
    bool read_done() { readt = now_s(); return rc == TDX_OK; }

    // one(ctx, stats): the host form tdx_x() on a context of its own, for one GPU.  strip(job, stats): tdx_x_strip() on the job's strip
    // arrays, for N GPUs; nullptr for a tool that has no strip form.
    template <class One, class Strip>
    bool compute(One one, Strip strip) {
        if constexpr (!std::is_same<Strip, std::nullptr_t>::value) {
            nproc = int(std::min<int64_t>(tool_gpus(), grid->info.ny));   // at least one row per rank
            if (nproc > 1) {
                rc = toolstrips::run(nproc, tool_device(), grid->info.nx, grid->info.ny, grid->info.dxc, grid->info.dyc, &st, strip);
                computet = now_s();
                return rc == TDX_OK;
            }
        }
        ctx.emplace();
        if (ctx->rc != TDX_OK) { rc = ctx->rc; return false; }
        rc = one(ctx->c, &st);
        if (rc != TDX_OK) { report(ctx->c); return false; }
        computet = now_s();
        return true;
    }

    template <class T>
    void output(const char* path, const std::vector<T>& data, const Raster& like, double nodata) {
        if (rc == TDX_OK) rc = save_raster(path, dtype_of<T>(), data.data(), like.info, nodata);
    }
    // midt: FlowDir only, the time at which the slope raster had been written.  stats_name == nullptr: no statistics line.
    int finish(const char* label, const char* stats_name, Footer footer = Footer::Times, double midt = 0.0) {
        if (rc != TDX_OK) return rc;
        const double writet = now_s(), slope_s = st.ms_kernel[TDX_K_STENCIL] / 1000.0;
        switch (footer) {
        case Footer::Times:
            printf("%s: %d\nRead time: %f\nCompute time: %f\nWrite time: %f\nTotal time: %f\n", label, nproc, readt - begint, computet - readt, writet - computet,
                   writet - begint);
            break;
        case Footer::HeaderTimes:
            printf("%s: %d\nHeader read time: %f\nData read time: %f\nCompute time: %f\nWrite time: %f\nTotal time: %f\n", label, nproc, 0.0, readt - begint,
                   computet - readt, writet - computet, writet - begint);
            break;
        case Footer::FlowDir:
            printf("%s: %d\nHeader read time: %f\nData read time: %f\nCompute Slope time: %f\nWrite Slope time: %f\nResolve Flat time: %f\nWrite Flat time: %f\nTotal time: %f\n",
                   label, nproc, 0.0, readt - begint, slope_s, midt - computet, (computet - readt) - slope_s, writet - midt, writet - begint);
            break;
        case Footer::CountOnly: printf("%s: %d\n", label, nproc); break;
        case Footer::ComputeOnly: printf("%s: %f\n", label, writet - begint); break;
        case Footer::NoWrite: printf("%s: %d\nRead time: %f\nCompute time: %f\nTotal time: %f\n", label, nproc, readt - begint, writet - readt, writet - begint); break;
        case Footer::ComputeWrite: printf("%s: %f\nFile write time: %f\n", label, computet - begint, writet - computet); break;
        case Footer::ComputeLine: printf("%s: %f\n", label, computet - readt); break;
        }
        if (stats_name) print_gpu_stats(stats_name, st, grid->info.nx * grid->info.ny);
        return 0;
    }
};

constexpr tdx::DType F32 = tdx::DType::F32, I16 = tdx::DType::I16, I32 = tdx::DType::I32;

}  // namespace

extern "C" {

int tdx_tool_set_device(int device) { g_tool_device = device; return TDX_OK; }
int tdx_tool_set_gpus(int ngpus) { g_tool_gpus = ngpus; return TDX_OK; }
int tdx_tool_set_streamnet_links(int where) {
    if (where != 0 && where != 1) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_set_streamnet_links: 0 (host) or 1 (device)");
    g_tool_streamnet_links = where;
    return TDX_OK;
}
int tdx_tool_set_polygon_rings(int where) {
    if (where != 0 && where != 1) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_set_polygon_rings: 0 (host) or 1 (device)");
    g_tool_polygon_rings = where;
    return TDX_OK;
}

int tdx_tool_pitremove(const char* demfile, const char* felfile, const char* /*sfdrfile*/, int /*usesfdr*/,
                       int verbose, int is_4Point, int use_mask, const char* maskfile) {
    ToolRun t("PitRemove");
    Raster dem, mask;
    t.input(demfile, F32, dem);
    if (use_mask) t.input(maskfile, I16, mask, Mismatch::PitRemove);
    if (!t.read_done()) return t.rc;
    if (verbose) { printf("Header read\nData read\n"); if (use_mask) printf("Process: 0, Using depression mask data...\n"); fflush(stdout); }
    std::vector<float> fel(t.cells());
    const float nd = (float)dem.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_pitremove(c, dem.f.data(), dem.info.nx, dem.info.ny, nd, use_mask ? mask.s.data() : nullptr, is_4Point, fel.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            float* d_dem = j.in(dem.f);
            int16_t* d_mask = use_mask ? j.in(mask.s) : nullptr;
            float* d_fel = j.out(fel);
            if (j.error) return j.error;
            return tdx_pitremove_strip(j.ctx, j.comm, d_dem, j.nx, j.nyl, nd, d_mask, is_4Point, d_fel, s);
        });
    if (!ok) return t.rc;
    if (verbose) printf("Process: 0, Pass: %lld, Remaining: 0\n", (long long)t.st.rounds);
    t.output(felfile, fel, dem, (double)-3.0e38f);   // felNodata
    return t.finish("Processes", "pitremove", Footer::HeaderTimes);
}

int tdx_tool_d8flowdir(const char* demfile, const char* pointfile, const char* slopefile, const char* /*flowfile*/, int useflowfile) {
    ToolRun t("D8FlowDir");
    if (useflowfile == 1) {
        // the reference's -sfdr branch reads an int32 partition through the int16 accessor and aborts
        // (src/d8.cpp:119,239-241 -> src/partition.h:100-107): treated as unsupported, same exit code
        printf("Attempt to access short grid with incorrect data type\n");
        return 41;
    }
    Raster dem;
    t.input(demfile, F32, dem);
    if (!t.read_done()) return t.rc;
    std::vector<int16_t> p(t.cells());
    std::vector<float> sd8(t.cells());
    const float nd = (float)dem.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_d8flowdir(c, dem.f.data(), dem.info.nx, dem.info.ny, nd, dem.info.dxc.data(), dem.info.dyc.data(), p.data(), sd8.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            float* d_fel = j.in(dem.f);
            int16_t* d_p = j.out(p);
            float* d_sd8 = j.out(sd8);
            if (j.error) return j.error;
            return tdx_d8flowdir_strip(j.ctx, j.comm, d_fel, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_p, d_sd8, s);
        });
    if (!ok) return t.rc;
    fprintf(stderr, "All slopes evaluated. %ld flats to resolve.\n", (long)t.st.flats_initial);
    if (t.st.flat_iterations > 0 && t.st.flats_left > 0) fprintf(stderr, "Iteration complete. Number of flats remaining: %ld\n", (long)t.st.flats_left);
    t.output(slopefile, sd8, dem, -1.0);
    const double writeSlopet = now_s();
    t.output(pointfile, p, dem, -32768.0);
    return t.finish("Processors", "d8flowdir", Footer::FlowDir, writeSlopet);
}

int tdx_tool_dinfflowdir(const char* demfile, const char* angfile, const char* slopefile, const char* /*flowfile*/, int /*useflowfile*/) {
    ToolRun t("DinfFlowDir");
    Raster dem;
    t.input(demfile, F32, dem);
    if (!t.read_done()) return t.rc;
    std::vector<float> ang(t.cells()), slp(t.cells());
    const float nd = (float)dem.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_dinfflowdir(c, dem.f.data(), dem.info.nx, dem.info.ny, nd, dem.info.dxc.data(), dem.info.dyc.data(), ang.data(), slp.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            float *d_fel = j.in(dem.f), *d_ang = j.out(ang), *d_slp = j.out(slp);
            if (j.error) return j.error;
            return tdx_dinfflowdir_strip(j.ctx, j.comm, d_fel, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_ang, d_slp, s);
        });
    if (!ok) return t.rc;
    fprintf(stderr, "All slopes evaluated. %ld flats to resolve.\n", (long)t.st.flats_initial);
    t.output(slopefile, slp, dem, -1.0);
    const double writeSlopet = now_s();
    t.output(angfile, ang, dem, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinfflowdir", Footer::FlowDir, writeSlopet);
}

int tdx_tool_aread8(const char* pfile, const char* afile, const char* datasrc, const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/,
                    const char* wfile, int useOutlets, int usew, int contcheck) {
    {   // existence probe of the reference (src/aread8.cpp:62-86)
        FILE* fp = fopen(pfile, "r");
        if (!fp) { fprintf(stderr, "Error: Input file %s does not exist.\n", pfile); return TDX_ERR_FILE; }
        fclose(fp);
    }
    ToolRun t("AreaD8");
    Raster p, w;
    Outlets o;
    t.input(pfile, I16, p);
    t.outlets(datasrc, useOutlets, o);
    if (usew == 1) t.input(wfile, F32, w);
    if (!t.read_done()) return t.rc;
    std::vector<float> a(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const float w_nd = usew ? (float)w.info.nodata : 0.f;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_aread8(c, p.s.data(), p.info.nx, p.info.ny, p_nd, usew ? w.f.data() : nullptr, w_nd, contcheck, o.xs(), o.ys(), o.n(), a.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            float* d_w = usew ? j.in(w.f) : nullptr;
            float* d_a = j.out(a);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_aread8_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_w, w_nd, contcheck, lo.xs(), lo.ys(), lo.n(), d_a, s);
        });
    if (!ok) return t.rc;
    t.output(afile, a, p, -1.0);
    return t.finish("Number of Processes", "aread8");
}

int tdx_tool_areadinf(const char* angfile, const char* scafile, const char* datasrc, const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/,
                      const char* wfile, int useOutlets, int usew, int contcheck) {
    ToolRun t("AreaDinf");
    Raster ang, w;
    Outlets o;
    t.input(angfile, F32, ang);
    t.outlets(datasrc, useOutlets, o);
    if (usew == 1) t.input(wfile, F32, w, Mismatch::Silent);   // src/areadinf.cpp:134
    if (!t.read_done()) return t.rc;
    std::vector<float> sca(t.cells());
    const float nd = (float)ang.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_areadinf(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), usew ? w.f.data() : nullptr, contcheck, o.xs(), o.ys(),
                                o.n(), sca.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float* d_ang = j.in(ang.f);
            float* d_w = usew ? j.in(w.f) : nullptr;
            float* d_out = j.out(sca);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_areadinf_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_w, contcheck, lo.xs(), lo.ys(), lo.n(), d_out, s);
        });
    if (!ok) return t.rc;
    t.output(scafile, sca, ang, -1.0);
    return t.finish("Processors", "areadinf");
}

int tdx_tool_dinfdecayaccum(const char* angfile, const char* adecfile, const char* dmfile, const char* datasrc, const char* /*lyrname*/,
                            int /*uselyrname*/, int /*lyrno*/, const char* wfile, int useOutlets, int usew, int contcheck) {
    ToolRun t("DinfDecayAccum");
    Raster ang, dm, w;
    Outlets o;
    t.input(angfile, F32, ang);
    t.outlets(datasrc, useOutlets, o);
    t.input(dmfile, F32, dm);
    if (usew == 1) t.input(wfile, F32, w);
    if (!t.read_done()) return t.rc;
    std::vector<float> out(t.cells());
    const float nd = (float)ang.info.nodata, dm_nd = (float)dm.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfdecayaccum(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), dm.f.data(), dm_nd, usew ? w.f.data() : nullptr,
                                      contcheck, o.xs(), o.ys(), o.n(), out.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_dm = j.in(dm.f);
            float* d_w = usew ? j.in(w.f) : nullptr;
            float* d_out = j.out(out);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_dinfdecayaccum_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_dm, dm_nd, d_w, contcheck, lo.xs(), lo.ys(), lo.n(), d_out, s);
        });
    if (!ok) return t.rc;
    t.output(adecfile, out, ang, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinfdecayaccum");
}

int tdx_tool_gridnet(const char* pfile, const char* plenfile, const char* tlenfile, const char* gordfile, const char* maskfile, const char* datasrc,
                     const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/, int useMask, int useOutlets, int thresh) {
    ToolRun t("GridNet");
    Raster p, mask;
    Outlets o;
    t.input(pfile, I16, p);
    t.outlets(datasrc, useOutlets, o);   // src/gridnet.cpp:78-120
    if (useMask == 1) t.input(maskfile, I32, mask);   // src/gridnet.cpp:147-152
    if (!t.read_done()) return t.rc;
    std::vector<float> plen(t.cells()), tlen(t.cells());
    std::vector<int16_t> gord(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_gridnet(c, p.s.data(), p.info.nx, p.info.ny, p_nd, p.info.dxc.data(), p.info.dyc.data(), useMask ? mask.l.data() : nullptr, thresh, o.xs(), o.ys(), o.n(),
                               plen.data(), tlen.data(), gord.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_m = useMask ? j.in(mask.l) : nullptr;
            float *d_pl = j.out(plen), *d_tl = j.out(tlen);
            int16_t* d_go = j.out(gord);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_gridnet_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, j.dxs.data(), j.dys.data(), d_m, thresh, lo.xs(), lo.ys(), lo.n(), d_pl, d_tl, d_go, s);
        });
    if (!ok) return t.rc;
    t.output(gordfile, gord, p, -1.0);   // src/gridnet.cpp:474-481
    t.output(plenfile, plen, p, -1.0);
    t.output(tlenfile, tlen, p, -1.0);
    return t.finish("Processors", "gridnet");
}

int tdx_tool_d8flowpathextremeup(const char* pfile, const char* safile, const char* ssafile, int usemax, const char* datasrc, const char* /*lyrname*/,
                                 int /*uselyrname*/, int /*lyrno*/, int useOutlets, int contcheck) {
    ToolRun t("D8FlowPathExtremeUp");
    Raster p, sa;
    Outlets o;
    t.input(pfile, I16, p);
    t.outlets(datasrc, useOutlets, o);
    t.input(safile, F32, sa);   // src/D8flowpathextremeup.cpp:120-125
    if (!t.read_done()) return t.rc;
    std::vector<float> ssa(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_d8flowpathextremeup(c, p.s.data(), p.info.nx, p.info.ny, p_nd, sa.f.data(), usemax, contcheck, o.xs(), o.ys(), o.n(), ssa.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            float *d_sa = j.in(sa.f), *d_out = j.out(ssa);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_d8flowpathextremeup_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_sa, usemax, contcheck, lo.xs(), lo.ys(), lo.n(), d_out, s);
        });
    if (!ok) return t.rc;
    t.output(ssafile, ssa, p, (double)TDX_ANG_NODATA);   // MISSINGFLOAT = -FLT_MAX (src/commonLib.h:80)
    return t.finish("Processors", "d8flowpathextremeup");
}

// One GPU whatever --gpus says: the tool has no strip form, and its footer says 1 (no statistics line).
int tdx_tool_threshold(const char* ssafile, const char* srcfile, const char* maskfile, float thresh, int usemask) {
    ToolRun t("Threshold");
    Raster ssa, mask;
    t.input(ssafile, F32, ssa);
    if (usemask == 1) t.input(maskfile, F32, mask, Mismatch::Silent);   // src/Threshold.cpp:90
    if (!t.read_done()) return t.rc;
    std::vector<int16_t> src(t.cells());
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_threshold(c, ssa.f.data(), ssa.info.nx, ssa.info.ny, (float)ssa.info.nodata, usemask ? mask.f.data() : nullptr, thresh, src.data(), s);
        },
        nullptr);
    if (!ok) return t.rc;
    t.output(srcfile, src, ssa, -32768.0);
    return t.finish("Processors", nullptr);
}

int tdx_tool_dinfupdependence(const char* angfile, const char* dgfile, const char* depfile) {
    ToolRun t("DinfUpDependence");
    Raster ang, dg;
    t.input(angfile, F32, ang);
    t.input(dgfile, I32, dg, Mismatch::Silent);   // src/DinfUpDependence.cpp:103
    if (!t.read_done()) return t.rc;
    std::vector<float> dep(t.cells());
    const float nd = (float)ang.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfupdependence(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), dg.l.data(), dep.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float* d_ang = j.in(ang.f);
            int32_t* d_dg = j.in(dg.l);
            float* d_dep = j.out(dep);
            if (j.error) return j.error;
            return tdx_dinfupdependence_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_dg, d_dep, s);
        });
    if (!ok) return t.rc;
    t.output(depfile, dep, ang, -1.0);   // depNodata = -1 (src/DinfUpDependence.cpp:113)
    return t.finish("Processors", "dinfupdependence");
}

int tdx_tool_dinfrevaccum(const char* angfile, const char* wgfile, const char* raccfile, const char* dmaxfile) {
    ToolRun t("DinfRevAccum");
    Raster ang, w;
    t.input(angfile, F32, ang);
    t.input(wgfile, F32, w);   // src/DinfRevAccum.cpp:94-99
    if (!t.read_done()) return t.rc;
    std::vector<float> racc(t.cells()), dmax(t.cells());
    const float nd = (float)ang.info.nodata, w_nd = (float)w.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfrevaccum(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), w.f.data(), w_nd, racc.data(), dmax.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_w = j.in(w.f), *d_r = j.out(racc), *d_m = j.out(dmax);
            if (j.error) return j.error;
            return tdx_dinfrevaccum_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_w, w_nd, d_r, d_m, s);
        });
    if (!ok) return t.rc;
    t.output(raccfile, racc, ang, (double)TDX_ANG_NODATA);   // MISSINGFLOAT (src/DinfRevAccum.cpp:253-258)
    t.output(dmaxfile, dmax, ang, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinfrevaccum");
}

int tdx_tool_dinfconclimaccum(const char* angfile, const char* ctptfile, const char* dmfile, const char* datasrc, const char* /*lyrname*/, int /*uselyrname*/,
                              int /*lyrno*/, const char* qfile, const char* dgfile, int useOutlets, int contcheck, float cSol) {
    ToolRun t("DinfConcLimAccum");
    Raster ang, dm, dg, q;
    Outlets o;
    t.input(angfile, F32, ang);
    t.outlets(datasrc, useOutlets, o);
    t.input(dmfile, F32, dm);
    t.input(dgfile, I16, dg);
    t.input(qfile, F32, q);
    if (!t.read_done()) return t.rc;
    std::vector<float> out(t.cells());
    const float nd = (float)ang.info.nodata, dm_nd = (float)dm.info.nodata, q_nd = (float)q.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfconclimaccum(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), dm.f.data(), dm_nd, dg.s.data(), q.f.data(), q_nd,
                                        cSol, contcheck, o.xs(), o.ys(), o.n(), out.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_dm = j.in(dm.f), *d_q = j.in(q.f);
            int16_t* d_dg = j.in(dg.s);
            float* d_out = j.out(out);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_dinfconclimaccum_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_dm, dm_nd, d_dg, d_q, q_nd, cSol, contcheck, lo.xs(), lo.ys(),
                                              lo.n(), d_out, s);
        });
    if (!ok) return t.rc;
    t.output(ctptfile, out, ang, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinfconclimaccum");
}

int tdx_tool_dinftranslimaccum(const char* angfile, const char* tsupfile, const char* tcfile, const char* tlafile, const char* depfile, const char* cinfile,
                               const char* coutfile, const char* datasrc, const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/, int useOutlets, int usec,
                               int contcheck) {
    ToolRun t("DinfTransLimAccum");
    Raster ang, tsup, tc, cin;
    Outlets o;
    t.input(angfile, F32, ang);
    t.outlets(datasrc, useOutlets, o);
    t.input(tsupfile, F32, tsup);
    t.input(tcfile, F32, tc);
    if (usec == 1) t.input(cinfile, F32, cin);
    if (!t.read_done()) return t.rc;
    std::vector<float> tla(t.cells()), dep(t.cells()), cso(usec ? t.cells() : 0);
    const float nd = (float)ang.info.nodata, ts_nd = (float)tsup.info.nodata, tc_nd = (float)tc.info.nodata, ci_nd = usec ? (float)cin.info.nodata : 0.f;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinftranslimaccum(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), tsup.f.data(), ts_nd, tc.f.data(), tc_nd,
                                         usec ? cin.f.data() : nullptr, ci_nd, contcheck, o.xs(), o.ys(), o.n(), tla.data(), dep.data(), usec ? cso.data() : nullptr, s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_ts = j.in(tsup.f), *d_tc = j.in(tc.f);
            float* d_ci = usec ? j.in(cin.f) : nullptr;
            float *d_tla = j.out(tla), *d_dep = j.out(dep);
            float* d_co = usec ? j.out(cso) : nullptr;
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            return tdx_dinftranslimaccum_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_ts, ts_nd, d_tc, tc_nd, d_ci, ci_nd, contcheck, lo.xs(), lo.ys(),
                                               lo.n(), d_tla, d_dep, d_co, s);
        });
    if (!ok) return t.rc;
    t.output(tlafile, tla, ang, (double)TDX_ANG_NODATA);
    t.output(depfile, dep, ang, (double)TDX_ANG_NODATA);
    if (usec == 1) t.output(coutfile, cso, ang, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinftranslimaccum");
}

// The four tool functions of each distance tool in one: files in the reference's order (ang, then fel for v / p / s, w for h / p / s when
// used - for v the weight code is commented out in the reference -, then src), each compared with ang; slpfile is never read.
static const char* const kDistType[4] = {"-h", "-v", "-p", "-s"};

int tdx_tool_dinfdistdown(const char* angfile, const char* felfile, const char* /*slpfile*/, const char* wfile, const char* srcfile, const char* dtsfile,
                          int statmethod, int typemethod, int usew, int concheck) {
    if (typemethod < 0 || typemethod > 3) return 0;   // (the reference's switch has no default: nothing runs)
    ToolRun t(std::string("DinfDistDown ") + kDistType[typemethod]);
    const bool use_fel = typemethod != 0, use_w = usew == 1 && typemethod != 1;
    Raster ang, fel, w, src;
    t.input(angfile, F32, ang);
    if (use_fel) t.input(felfile, F32, fel);
    if (use_w) t.input(wfile, F32, w);
    t.input(srcfile, I16, src);
    if (!t.read_done()) return t.rc;
    std::vector<float> dd(t.cells());
    const float nd = (float)ang.info.nodata, fel_nd = use_fel ? (float)fel.info.nodata : 0.f, w_nd = use_w ? (float)w.info.nodata : 0.f;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfdistdown(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), use_fel ? fel.f.data() : nullptr, fel_nd, src.s.data(),
                                    use_w ? w.f.data() : nullptr, w_nd, statmethod, typemethod, concheck, dd.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float* d_ang = j.in(ang.f);
            float* d_fel = use_fel ? j.in(fel.f) : nullptr;
            float* d_w = use_w ? j.in(w.f) : nullptr;
            int16_t* d_src = j.in(src.s);
            float* d_dd = j.out(dd);
            if (j.error) return j.error;
            return tdx_dinfdistdown_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_fel, fel_nd, d_src, d_w, w_nd, statmethod, typemethod, concheck, d_dd, s);
        });
    if (!ok) return t.rc;
    t.output(dtsfile, dd, ang, (double)TDX_ANG_NODATA);   // MISSINGFLOAT (src/DinfDistDown.cpp:363-365)
    return t.finish("Processors", "dinfdistdown");
}

int tdx_tool_dinfdistup(const char* angfile, const char* felfile, const char* /*slpfile*/, const char* wfile, const char* rtrfile, int statmethod,
                        int typemethod, int usew, int concheck, float thresh) {
    if (typemethod < 0 || typemethod > 3) return 0;   // (the reference's switch has no default: nothing runs)
    ToolRun t(std::string("DinfDistUp ") + kDistType[typemethod]);
    const bool use_fel = typemethod != 0, use_w = usew == 1 && typemethod != 1;
    Raster ang, fel, w;
    t.input(angfile, F32, ang);
    if (use_fel) t.input(felfile, F32, fel);
    if (use_w) t.input(wfile, F32, w);
    if (!t.read_done()) return t.rc;
    std::vector<float> du(t.cells());
    const float nd = (float)ang.info.nodata, fel_nd = use_fel ? (float)fel.info.nodata : 0.f, w_nd = use_w ? (float)w.info.nodata : 0.f;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfdistup(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), use_fel ? fel.f.data() : nullptr, fel_nd,
                                  use_w ? w.f.data() : nullptr, w_nd, statmethod, typemethod, concheck, thresh, du.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float* d_ang = j.in(ang.f);
            float* d_fel = use_fel ? j.in(fel.f) : nullptr;
            float* d_w = use_w ? j.in(w.f) : nullptr;
            float* d_du = j.out(du);
            if (j.error) return j.error;
            return tdx_dinfdistup_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_fel, fel_nd, d_w, w_nd, statmethod, typemethod, concheck, thresh, d_du, s);
        });
    if (!ok) return t.rc;
    t.output(rtrfile, du, ang, (double)TDX_ANG_NODATA);   // MISSINGFLOAT (src/DinfDistUp.cpp:321-322)
    return t.finish("Processors", "dinfdistup");
}

// ang, wg, rc, each compared with ang; the output header is rc's
int tdx_tool_retlimflow(const char* angfile, const char* wgfile, const char* rcfile, const char* qrlfile) {
    ToolRun t("Retention limited flow accumulation");
    Raster ang, wg, rcg;
    t.input(angfile, F32, ang);
    t.input(wgfile, F32, wg);
    t.input(rcfile, F32, rcg);
    if (!t.read_done()) return t.rc;
    std::vector<float> qrl(t.cells());
    const float nd = (float)ang.info.nodata, wg_nd = (float)wg.info.nodata, rc_nd = (float)rcg.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_retlimflow(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), wg.f.data(), wg_nd, rcg.f.data(), rc_nd, qrl.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_wg = j.in(wg.f), *d_rc = j.in(rcg.f), *d_q = j.out(qrl);
            if (j.error) return j.error;
            return tdx_retlimflow_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_wg, wg_nd, d_rc, rc_nd, d_q, s);
        });
    if (!ok) return t.rc;
    t.output(qrlfile, qrl, rcg, (double)TDX_ANG_NODATA);   // MISSINGFLOAT, header of rc (src/RetlimFlow.cpp:233-235)
    return t.finish("Processors", "retlimflow", Footer::CountOnly);
}

// ang, fel, ass (SHORT), each compared with ang.  -direct reads the file's coordinates: the geotransform goes to the library.
int tdx_tool_dinfavalanche(const char* angfile, const char* felfile, const char* assfile, const char* rzfile, const char* dmfile, float thresh, float alpha, int path) {
    ToolRun t("DinfAvalanche");
    Raster ang, fel, ass;
    t.input(angfile, F32, ang);
    t.input(felfile, F32, fel, Mismatch::Avalanche);
    t.input(assfile, I16, ass, Mismatch::Avalanche);
    if (!t.read_done()) return t.rc;
    std::vector<float> rz(t.cells()), dfs(t.cells());
    const double geo[4] = {ang.info.xleftedge, ang.info.ytopedge, ang.info.dlon, ang.info.dlat};
    const int geographic = ang.info.geographic ? 1 : 0;
    const float nd = (float)ang.info.nodata, fel_nd = (float)fel.info.nodata;
    const int16_t ass_nd = (int16_t)ass.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dinfavalanche(c, ang.f.data(), ang.info.nx, ang.info.ny, nd, ang.info.dxc.data(), ang.info.dyc.data(), fel.f.data(), fel_nd, ass.s.data(), ass_nd, thresh, alpha,
                                     path, geo, geographic, rz.data(), dfs.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_ang = j.in(ang.f), *d_fel = j.in(fel.f);
            int16_t* d_ass = j.in(ass.s);
            float *d_rz = j.out(rz), *d_dfs = j.out(dfs);
            if (j.error) return j.error;
            return tdx_dinfavalanche_strip(j.ctx, j.comm, d_ang, j.nx, j.nyl, nd, j.dxs.data(), j.dys.data(), d_fel, fel_nd, d_ass, ass_nd, thresh, alpha, path, geo, geographic, j.y0,
                                           j.ny, d_rz, d_dfs, s);
        });
    if (!ok) return t.rc;
    t.output(rzfile, rz, ang, (double)TDX_ANG_NODATA);   // MISSINGFLOAT, header of ang (src/DinfAvalanche.cpp:384-389)
    t.output(dmfile, dfs, ang, (double)TDX_ANG_NODATA);
    return t.finish("Processors", "dinfavalanche");
}

// p, then src read as LONG
int tdx_tool_d8hdisttostrm(const char* pfile, const char* srcfile, const char* distfile, int thresh) {
    ToolRun t("D8HDistToStrm");
    Raster p, src;
    t.input(pfile, I16, p);
    t.input(srcfile, I32, src);
    if (!t.read_done()) return t.rc;
    std::vector<float> dist(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const int32_t s_nd = (int32_t)src.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_d8hdisttostrm(c, p.s.data(), p.info.nx, p.info.ny, p_nd, src.l.data(), s_nd, thresh, p.info.dxc.data(), p.info.dyc.data(), dist.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_src = j.in(src.l);
            float* d_dist = j.out(dist);
            if (j.error) return j.error;
            return tdx_d8hdisttostrm_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_src, s_nd, thresh, j.dxs.data(), j.dys.data(), d_dist, s);
        });
    if (!ok) return t.rc;
    t.output(distfile, dist, p, (double)TDX_ANG_NODATA);   // MISSINGFLOAT (src/D8HDistToStrm.cpp:223-225)
    return t.finish("Processors", "d8hdisttostrm");
}

// StreamNet (src/streamnet.cpp:372-1508): reads src, p, ad8, fel in the reference's order with its own words for a raster that does not match (it
// aborts with 4), then the outlets.  -lyrname / -lyrno are accepted and ignored, as for the other outlet tools.  The -net flag is still refused here;
// the layer itself - every one of its fields is a host function of the tree and coord rows (reachshape, :244-365) - is written by
// tdx_streamnet_net_write from the links of tdx_streamnet.
int tdx_tool_streamnet(const char* pfile, const char* srcfile, const char* ordfile, const char* ad8file, const char* elevfile, const char* treefile,
                       const char* coordfile, const char* outletsds, const char* /*lyrname*/, int /*uselayername*/, int /*lyrno*/, const char* wfile,
                       const char* streamnetsrc, const char* streamnetlyr, long useOutlets, long ordert, int verbose) {
    if ((streamnetsrc && *streamnetsrc) || (streamnetlyr && *streamnetlyr)) {
        fprintf(stderr, "taudem_amd: streamnet -net / -netlyr are not supported (the stream network layer is not written)\n");
        g_tdx_thread_error = "streamnet: -net is not supported";
        return TDX_ERR_ARG;
    }
    ToolRun t("StreamNet");
    Raster src, p, ad8, fel;
    Outlets o;
    t.input(srcfile, I16, src);
    if (t.rc == TDX_OK) {
        const float timeestimate = float(1e-4 * double(src.info.nx) * double(src.info.ny) / 60 + 1);   // the reference's words and its estimate for one rank (:408-410)
        fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
        fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
        fflush(stderr);
    }
    const struct { const char* path; tdx::DType type; Raster* r; const char* what; } more[3] = {
        {pfile, I16, &p, "pfile"}, {ad8file, F32, &ad8, "ad8file"}, {elevfile, F32, &fel, "elevfile"}};
    for (const auto& m : more) {
        t.input(m.path, m.type, *m.r, Mismatch::Silent);
        if (t.rc == TDX_ERR_MISMATCH) { printf("%s and src files not the same size. Exiting \n", m.what); fflush(stdout); return 4; }
    }
    if (useOutlets == 1) {
        t.outlets(outletsds, 1, o);
        if (t.rc == TDX_ERR_OUTLETS) { printf("Read outlets error. Exiting \n"); fflush(stdout); return t.rc; }
    }
    if (!t.read_done()) return t.rc;
    const int64_t nx = src.info.nx, ny = src.info.ny, nout = useOutlets == 1 ? o.n() : 0;
    if (verbose) {
        printf("Files read\nProcess: 0, TotalX: %ld, TotalY: %ld\nProcess: 0, nx: %d, ny: %d\nProcess: 0, xstart: 0, ystart: 0\nProcess: 0, numOutlets: %d\n", long(nx), long(ny),
               int(nx), int(ny), int(nout));
        fflush(stdout);
    }
    fprintf(stderr, "Evaluating distances to outlet\nCreating links\n");   // (one call makes both: the reference's progress lines, ahead of it)
    fflush(stderr);
    std::vector<int32_t> src32(src.s.begin(), src.s.end()), w(t.cells());
    std::vector<int16_t> ord(t.cells());
    const double gt[4] = {src.info.xleftedge, src.info.dlon, src.info.ytopedge, src.info.dlat};
    const int16_t p_nd = (int16_t)p.info.nodata;
    const int32_t src_nd = (int32_t)(int16_t)src.info.nodata;
    const int sw = ordert == 0;
    tdx_streamnet_links* links = nullptr;
    // --gpus N: every rank compacts its strip, the ranks meet, rank 0 builds the links of the whole raster (on the host, or after
    // tdx_tool_set_streamnet_links(1) on its device), they meet again, every rank labels
    // its strip.  A rank that fails still comes to both meetings, so that nobody waits there for it.
    const int nranks = int(std::min<int64_t>(tool_gpus(), ny));
    std::vector<tdx_streamnet_compact*> parts(size_t(std::max(nranks, 1)), nullptr);
    struct Meet {
        std::mutex m; std::condition_variable cv; int n = 1, here = 0, round = 0;
        void wait() {
            std::unique_lock<std::mutex> lk(m);
            const int r = round;
            if (++here == n) { here = 0; round++; cv.notify_all(); } else cv.wait(lk, [&] { return round != r; });
        }
    } meet;
    meet.n = std::max(nranks, 1);
    std::atomic<int> failed{0};
    const bool device_links = g_tool_streamnet_links == 1;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return (device_links ? tdx_streamnet_gpu_links : tdx_streamnet)(c, p.s.data(), src32.data(), fel.f.data(), ad8.f.data(), nx, ny, p_nd, src_nd, src.info.dxc.data(), src.info.dyc.data(), src.info.dxA(),
                                 src.info.dyA(), gt, nout ? o.xs() : nullptr, nout ? o.ys() : nullptr, nout ? o.ids.data() : nullptr, nout, sw, ord.data(), w.data(), &links, s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_s = j.in(src32);
            float *d_f = j.in(fel.f), *d_a = j.in(ad8.f);
            int16_t* d_o = j.out(ord);
            int32_t* d_w = j.out(w);
            int e = j.error;
            if (e == TDX_OK) e = tdx_streamnet_compact_strip(j.ctx, j.comm, d_p, d_s, d_f, d_a, j.nx, j.nyl, j.y0, p_nd, src_nd, j.dxs.data(), j.dys.data(), &parts[size_t(j.rank)], s);
            if (e != TDX_OK) failed = e;
            meet.wait();
            if (failed == 0 && j.rank == 0) {
                const int eb = device_links ? tdx_streamnet_links_build_gpu(j.ctx, parts.data(), j.size, nx, ny, src.info.dxA(), src.info.dyA(), gt, nout ? o.xs() : nullptr,
                                                                            nout ? o.ys() : nullptr, nout ? o.ids.data() : nullptr, nout, &links)
                                            : tdx_streamnet_links_build(parts.data(), j.size, nx, ny, src.info.dxA(), src.info.dyA(), gt, nout ? o.xs() : nullptr,
                                                                        nout ? o.ys() : nullptr, nout ? o.ids.data() : nullptr, nout, &links);
                if (eb != TDX_OK) failed = eb;
            }
            meet.wait();
            if (failed != 0) return e != TDX_OK ? e : int(failed);
            int64_t first_cell = 0;
            for (int k = 0; k < j.rank; k++) first_cell += tdx_streamnet_compact_count(parts[size_t(k)]);
            return tdx_streamnet_label_strip(j.ctx, j.comm, d_p, d_s, j.nx, j.nyl, p_nd, src_nd, parts[size_t(j.rank)], links, first_cell, sw, d_o, d_w, s);
        });
    for (tdx_streamnet_compact* part : parts) tdx_streamnet_compact_free(part);
    if (!ok) { tdx_streamnet_links_free(links); return t.rc; }
    double phase[TDX_STREAMNET_PHASES];
    tdx_streamnet_links_copy(links, nullptr, nullptr, phase);
    int wrc = tdx_streamnet_write_text(links, treefile, nullptr);
    const char* failed_file = treefile;
    if (wrc == TDX_OK) { wrc = tdx_streamnet_write_text(links, nullptr, coordfile); failed_file = coordfile; }
    tdx_streamnet_links_free(links);
    if (wrc != TDX_OK) { printf("Error opening file %s.\n", failed_file); fflush(stdout); return wrc; }
    const double linkwt = now_s();
    fprintf(stderr, "\n Calculating watersheds\n");
    fflush(stderr);
    t.output(wfile, w, ad8, -2147483647.0);    // MISSINGLONG, written like ad8 (:1450-1453)
    t.output(ordfile, ord, ad8, -32768.0);     // MISSINGSHORT (:1473)
    if (t.rc != TDX_OK) return t.rc;
    const double writet = now_s();
    const double lengthc = (phase[TDX_STREAMNET_SETUP] + phase[TDX_STREAMNET_LENGTH]) / 1000.0,
                 linkc = (phase[TDX_STREAMNET_COMPACT] + phase[TDX_STREAMNET_LINKS]) / 1000.0,
                 wshed = (phase[TDX_STREAMNET_SCATTER] + phase[TDX_STREAMNET_LABEL]) / 1000.0;
    printf("Processors: %d\nRead time: %f\nLength compute time: %f\nLink compute time: %f\nLink write time: %f\nWatershed compute time: %f\nWrite time: %f\nTotal time: %f\n",
           t.nproc, t.readt - t.begint, lengthc, linkc, linkwt - t.computet, wshed, writet - linkwt, writet - t.begint);
    print_gpu_stats("streamnet", t.st, nx * ny);
    return 0;
}

// -lyrname / -lyrno are accepted and ignored, as for the other outlet tools.  -upid is refused: the reference appends a line per visit of a
// nodata neighbour in queue order (src/gagewatershed.cpp:246-253), which depends on the schedule.
int tdx_tool_gagewatershed(const char* pfile, const char* wfile, const char* datasrc, const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/,
                           const char* idfile, int writeid, int writeupid, const char* /*upidfile*/) {
    ToolRun t("Gage Watershed");
    if (writeupid == 1) {
        fprintf(stderr, "taudem_amd: gagewatershed -upid is not supported (the reference's upstream-id file depends on its queue order)\n");
        g_tdx_thread_error = "gagewatershed: -upid is not supported";
        return TDX_ERR_ARG;
    }
    Raster p;
    Outlets o;
    t.input(pfile, I16, p);
    t.outlets(datasrc, 1, o);
    if (!t.read_done()) return t.rc;
    const int64_t nout = o.n();
    std::vector<int32_t> gw(t.cells()), placed(size_t(nout) + 1), iddown(size_t(nout) + 1);
    const int16_t p_nd = (int16_t)p.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_gagewatershed(c, p.s.data(), p.info.nx, p.info.ny, p_nd, o.xs(), o.ys(), o.ids.data(), nout, gw.data(), placed.data(), iddown.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_gw = j.out(gw);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            std::vector<int32_t> pl(size_t(nout) + 1), dn(size_t(nout) + 1);   // (every rank gets the reduced table: rank 0's is kept)
            const int e = tdx_gagewatershed_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, lo.xs(), lo.ys(), o.ids.data(), nout, d_gw, pl.data(), dn.data(), s);
            if (e == TDX_OK && j.rank == 0) { placed = pl; iddown = dn; }
            return e;
        });
    if (!ok) return t.rc;
    if (writeid == 1) {   // before the raster (src/gagewatershed.cpp:327-341)
        FILE* f = fopen(idfile, "w");
        if (!f) { printf("Error opening file %s.\n", idfile); fflush(stdout); return TDX_ERR_FILE; }
        fprintf(f, "id iddown\n");
        for (int64_t i = 0; i < nout; i++)
            if (placed[size_t(i)] > 0) fprintf(f, "%d %d\n", o.ids[size_t(i)], iddown[size_t(i)]);
        fclose(f);
    }
    t.output(wfile, gw, p, -2147483647.0);   // MISSINGLONG (src/gagewatershed.cpp:346-348)
    return t.finish("Size", "gagewatershed");
}

// p, then z; the output is written like z, with z's nodata value (src/flowdircond.cpp:224)
int tdx_tool_flowdircond(const char* pfile, const char* zfile, const char* zfdcfile) {
    ToolRun t("FlowDirCond");
    Raster p, z;
    t.input(pfile, I16, p);
    t.input(zfile, F32, z);
    if (!t.read_done()) return t.rc;
    std::vector<float> out(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const float z_nd = (float)z.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_flowdircond(c, p.s.data(), p.info.nx, p.info.ny, p_nd, z.f.data(), z_nd, out.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            float *d_z = j.in(z.f), *d_o = j.out(out);
            if (j.error) return j.error;
            return tdx_flowdircond_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_z, z_nd, d_o, s);
        });
    if (!ok) return t.rc;
    t.output(zfdcfile, out, z, z.info.nodata);
    return t.finish("Processors", "flowdircond");
}

// p, fel, then src read as LONG
int tdx_tool_d8vdisttostrm(const char* pfile, const char* felfile, const char* srcfile, const char* distfile, int thresh) {
    ToolRun t("D8VDistToStrm");
    Raster p, fel, src;
    t.input(pfile, I16, p);
    t.input(felfile, F32, fel);
    t.input(srcfile, I32, src);
    if (!t.read_done()) return t.rc;
    std::vector<float> dist(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const int32_t s_nd = (int32_t)src.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_d8vdisttostrm(c, p.s.data(), p.info.nx, p.info.ny, p_nd, fel.f.data(), src.l.data(), s_nd, thresh, dist.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            float* d_fel = j.in(fel.f);
            int32_t* d_src = j.in(src.l);
            float* d_dist = j.out(dist);
            if (j.error) return j.error;
            return tdx_d8vdisttostrm_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_fel, d_src, s_nd, thresh, d_dist, s);
        });
    if (!ok) return t.rc;
    t.output(distfile, dist, p, (double)TDX_ANG_NODATA);   // MISSINGFLOAT (src/D8VDistToStrm.cpp:250-252)
    return t.finish("Processors", "d8vdisttostrm");
}

// fel first, then p compared with it: the cell sizes are fel's, the output is written like p.  niter = int(dn / min(dxA, dyA)) + 1
// (src/SlopeAveDown.cpp:172) is not capped; a dn that is negative or not finite is refused.
int tdx_tool_slopeavedown(const char* pfile, const char* felfile, const char* slpdfile, double dn) {
    ToolRun t("SlopeAveDown");
    if (!std::isfinite(dn) || dn < 0.0) {
        fprintf(stderr, "taudem_amd: slopeavedown: dn must be finite and not negative\n");
        g_tdx_thread_error = "slopeavedown: dn must be finite and not negative";
        return TDX_ERR_ARG;
    }
    Raster p, fel;
    t.input(felfile, F32, fel);
    t.input(pfile, I16, p);
    if (!t.read_done()) return t.rc;
    const int64_t niter = tdx_slopeavedown_niter(dn, fel.info.dxc.data(), fel.info.dyc.data(), fel.info.ny);
    if (niter <= 0) { g_tdx_thread_error = "slopeavedown: the cell sizes give no iteration count"; return TDX_ERR_ARG; }
    fprintf(stderr, "Number of slope down interations to do %lld\n", (long long)niter);
    fflush(stderr);
    std::vector<float> sd(t.cells());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const float f_nd = (float)fel.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_slopeavedown(c, p.s.data(), p.info.nx, p.info.ny, p_nd, fel.f.data(), f_nd, fel.info.dxc.data(), fel.info.dyc.data(), dn, niter, sd.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            float *d_fel = j.in(fel.f), *d_sd = j.out(sd);
            if (j.error) return j.error;
            return tdx_slopeavedown_strip(j.ctx, j.comm, d_p, j.nx, j.nyl, p_nd, d_fel, f_nd, j.dxs.data(), j.dys.data(), dn, niter, d_sd, s);
        });
    if (!ok) return t.rc;
    t.output(slpdfile, sd, p, (double)TDX_ANG_NODATA);   // MISSINGFLOAT, like pIO (src/SlopeAveDown.cpp:302-304)
    return t.finish("Processors", "slopeavedown");
}

// hand, catch (LONG), slp, each compared with hand: a mismatch returns 1 without a word.  Then the catchment list and the stage file; a list that cannot be
// used ends the run with the reference's message and 1 (the reference calls exit(1) there).  With N GPUs every strip returns its own sums and they are
// added here in strip order.
int tdx_tool_catchhydrogeo(const char* handfile, const char* catchfile, const char* catchlistfile, const char* slpfile, const char* hfile, const char* hpfile) {
    ToolRun t("CatchHydroGeo");
    Raster hand, cat, slp;
    t.input(handfile, F32, hand);
    t.input(catchfile, I32, cat, Mismatch::Silent);
    t.input(slpfile, F32, slp, Mismatch::Silent);
    if (!t.read_done()) return t.rc;
    handtables::CatchList cl;
    std::vector<double> stage;
    if (!handtables::read_catch_list(catchlistfile, cl)) return 1;
    if (!handtables::read_stages(hfile, stage)) { fprintf(stderr, "taudem_amd: cannot open stage file %s\n", hfile); return TDX_ERR_FILE; }
    const int64_t nc = int64_t(cl.id.size()), nh = int64_t(stage.size());
    const size_t nt = size_t(nc) * size_t(nh);
    struct Sums {
        std::vector<int32_t> count;
        std::vector<double> surface, bed, volume, area;
        void size(size_t nt, size_t nc) { count.assign(nt, 0); surface.assign(nt, 0.0); bed.assign(nt, 0.0); volume.assign(nt, 0.0); area.assign(nc, 0.0); }
    } total;
    total.size(nt, size_t(nc));
    std::vector<Sums> part(size_t(std::max(tool_gpus(), 1)));
    const float h_nd = (float)hand.info.nodata, s_nd = (float)slp.info.nodata;
    const int32_t c_nd = (int32_t)cat.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_catchhydrogeo(c, hand.f.data(), cat.l.data(), slp.f.data(), hand.info.nx, hand.info.ny, h_nd, c_nd, s_nd, hand.info.dxc.data(), hand.info.dyc.data(),
                                     cl.id.data(), nc, stage.data(), nh, total.count.data(), total.surface.data(), total.bed.data(), total.volume.data(), total.area.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_h = j.in(hand.f), *d_s = j.in(slp.f);
            int32_t* d_c = j.in(cat.l);
            if (j.error) return j.error;
            Sums& p = part[size_t(j.rank)];
            p.size(nt, size_t(nc));
            return tdx_catchhydrogeo_strip(j.ctx, j.comm, d_h, d_c, d_s, j.nx, j.nyl, h_nd, c_nd, s_nd, j.dxs.data(), j.dys.data(), cl.id.data(), nc, stage.data(), nh,
                                           p.count.data(), p.surface.data(), p.bed.data(), p.volume.data(), p.area.data(), s);
        });
    if (!ok) return t.rc;
    if (t.nproc > 1)
        for (int r = 0; r < t.nproc; r++) {   // strip order: fixed
            const Sums& p = part[size_t(r)];
            for (size_t i = 0; i < nt; i++) { total.count[i] += p.count[i]; total.surface[i] += p.surface[i]; total.bed[i] += p.bed[i]; total.volume[i] += p.volume[i]; }
            for (size_t i = 0; i < size_t(nc); i++) total.area[i] += p.area[i];
        }
    if (!handtables::write_hydroprop(hpfile, cl, stage, total.count, total.surface, total.bed, total.volume, total.area)) {
        printf("Error opening file %s.\n", hpfile);
        fflush(stdout);
        return TDX_ERR_FILE;
    }
    return t.finish("Compute time", "catchhydrogeo", Footer::ComputeOnly);
}

// hand, catch (LONG), the mask (SHORT) when given, each compared with hand: a mismatch returns 1 without a word.  maskfile / depthfile: NULL or "" when
// not given.  With a mask the depth raster is nodata everywhere, as in the reference (its line 465); the depth CSV is not affected.
int tdx_tool_inundepth(const char* handfile, const char* catchfile, const char* maskfile, const char* fcfile, const char* hpfile, const char* mapfile, const char* depthfile) {
    ToolRun t("InunDepth");
    const bool use_mask = maskfile && *maskfile, want_depths = depthfile && *depthfile;
    Raster hand, cat, mask;
    t.input(handfile, F32, hand);
    t.input(catchfile, I32, cat, Mismatch::Silent);
    if (use_mask) t.input(maskfile, I16, mask, Mismatch::Silent);
    if (!t.read_done()) return t.rc;
    handtables::Forecast fc;
    if (!handtables::read_forecast(fcfile, hpfile, fc)) return 1;
    const int64_t nfc = int64_t(fc.id.size());
    std::vector<float> map(t.cells()), area(want_depths ? size_t(nfc) : 0);
    std::vector<std::vector<double>> part(size_t(std::max(tool_gpus(), 1)));
    const float h_nd = (float)hand.info.nodata;
    const int32_t c_nd = (int32_t)cat.info.nodata;
    const int16_t m_nd = use_mask ? (int16_t)mask.info.nodata : int16_t(0);
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_inundepth(c, hand.f.data(), cat.l.data(), use_mask ? mask.s.data() : nullptr, hand.info.nx, hand.info.ny, h_nd, c_nd, m_nd, hand.info.dxc.data(),
                                 hand.info.dyc.data(), fc.id.data(), fc.depth.data(), nfc, map.data(), want_depths ? area.data() : nullptr, s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float* d_h = j.in(hand.f);
            int32_t* d_c = j.in(cat.l);
            int16_t* d_m = use_mask ? j.in(mask.s) : nullptr;
            float* d_map = j.out(map);
            if (j.error) return j.error;
            std::vector<double>& p = part[size_t(j.rank)];
            if (want_depths) p.assign(size_t(nfc), 0.0);
            return tdx_inundepth_strip(j.ctx, j.comm, d_h, d_c, d_m, j.nx, j.nyl, h_nd, c_nd, m_nd, j.dxs.data(), j.dys.data(), fc.id.data(), fc.depth.data(), nfc, d_map,
                                       want_depths ? p.data() : nullptr, s);
        });
    if (!ok) return t.rc;
    if (want_depths) {
        if (t.nproc > 1)
            for (size_t i = 0; i < size_t(nfc); i++) {
                double sum = 0.0;
                for (int r = 0; r < t.nproc; r++) sum += part[size_t(r)][i];   // strip order, rounded once
                area[i] = float(sum);
            }
        handtables::write_depths(depthfile, fc, area);
    }
    t.output(mapfile, map, hand, (double)-3.0e38f);   // felNodata, header of hand (src/InunDepth.cpp:446,521)
    return t.finish("Inundation depth Compute time", "inundepth", Footer::ComputeOnly);
}

// ssa first, then p and ad8, each compared as the reference compares them (its messages, its codes 4 and 5), the outlets, then fel.  An outlet on a cell
// without a direction is refused before anything runs (the reference indexes outside its offset table there).  With N GPUs every strip returns its own
// counts, sums and length, which are added here in strip order; the outlets' terms of the total area are added in file order.
int tdx_tool_dropanalysis(const char* areafile, const char* dirfile, const char* elevfile, const char* ssafile, const char* dropfile, const char* datasrc,
                          const char* /*lyrname*/, int /*uselyrname*/, int /*lyrno*/, float threshmin, float threshmax, int nthresh, int steptype, float* threshopt) {
    ToolRun t("DropAnalysis");
    Raster ssa, p, ad8, fel;
    Outlets o;
    t.input(ssafile, F32, ssa);
    if (t.rc == TDX_OK) {   // src/DropAnalysis.cpp:207-213
        const float timeestimate = (2e-7 * ssa.info.nx * ssa.info.ny * nthresh / pow((double)tool_gpus(), 0.65)) / 60 + 1;
        fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
        fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the "
                        "computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
        fflush(stderr);
    }
    t.input(dirfile, I16, p, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("dir and ssa files not the same size. Exiting \n"); fflush(stdout); return 4; }
    t.input(areafile, F32, ad8, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("ssa and area files not the same size. Exiting \n"); fflush(stdout); return 4; }
    t.outlets(datasrc ? datasrc : "", 1, o);
    t.input(elevfile, F32, fel, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("elev and ssa files not the same size. Exiting \n"); fflush(stdout); return 5; }
    if (!t.read_done()) return t.rc;
    if (nthresh < 2) { printf("Number of thresholds must be greater than 1. \n"); fflush(stdout); return 7; }   // src/DropAnalysis.cpp:369-373
    const int64_t nx = ssa.info.nx, ny = ssa.info.ny, nout = int64_t(o.x.size());
    const int16_t p_nd = (int16_t)p.info.nodata;
    const float ssa_nd = (float)ssa.info.nodata;
    for (int64_t i = 0; i < nout; i++) {
        if (o.x[size_t(i)] < 0 || o.x[size_t(i)] >= nx || o.y[size_t(i)] < 0 || o.y[size_t(i)] >= ny) continue;
        const int16_t d = p.s[size_t(o.y[size_t(i)]) * size_t(nx) + size_t(o.x[size_t(i)])];
        if (d == p_nd || d < 0 || d > 8) {
            fprintf(stderr, "taudem_amd: outlet %lld (column %d, row %d) lies on a cell without a flow direction\n", (long long)i, int(o.x[size_t(i)]), int(o.y[size_t(i)]));
            return TDX_ERR_ARG;
        }
    }
    struct Part {
        std::vector<float> thresh, term;
        std::vector<int64_t> n1, n2;
        std::vector<double> sums, length;
        void size(size_t nt, size_t no) { thresh.assign(nt, 0.f); term.assign(no, 0.f); n1.assign(nt, 0); n2.assign(nt, 0); sums.assign(4 * nt, 0.0); length.assign(nt, 0.0); }
    } total;
    const size_t nt = size_t(nthresh);
    total.size(nt, size_t(nout));
    std::vector<Part> part(size_t(std::max(tool_gpus(), 1)));
    float total_area = 0.f;
    const double dxA = ad8.info.dxA(), dyA = ad8.info.dyA();
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_dropanalysis(c, ad8.f.data(), p.s.data(), fel.f.data(), ssa.f.data(), nx, ny, p_nd, ssa_nd, ssa.info.dxc.data(), ssa.info.dyc.data(), dxA, dyA, o.xs(),
                                    o.ys(), nout, threshmin, threshmax, nthresh, steptype, -1, nullptr, nullptr, total.thresh.data(), total.n1.data(), total.n2.data(),
                                    total.sums.data(), total.length.data(), &total_area, nullptr, nullptr, nullptr, 0, s);
        },
        [&](RankJob& j, tdx_stats* s) {
            float *d_a = j.in(ad8.f), *d_f = j.in(fel.f), *d_s = j.in(ssa.f);
            int16_t* d_p = j.in(p.s);
            if (j.error) return j.error;
            const toolstrips::LocalOutlets lo = j.local(o);
            Part& q = part[size_t(j.rank)];
            q.size(nt, size_t(nout));
            return tdx_dropanalysis_strip(j.ctx, j.comm, d_a, d_p, d_f, d_s, j.nx, j.nyl, p_nd, ssa_nd, j.dxs.data(), j.dys.data(), lo.xs(), lo.ys(), nout, threshmin, threshmax,
                                          nthresh, steptype, -1, nullptr, nullptr, q.thresh.data(), q.n1.data(), q.n2.data(), q.sums.data(), q.length.data(), q.term.data(), s);
        });
    if (!ok) return t.rc;
    if (t.nproc > 1) {
        total.thresh = part[0].thresh;
        for (int r = 0; r < t.nproc; r++) {   // strip order: fixed
            const Part& q = part[size_t(r)];
            for (size_t i = 0; i < nt; i++) { total.n1[i] += q.n1[i]; total.n2[i] += q.n2[i]; total.length[i] += q.length[i]; }
            for (size_t i = 0; i < 4 * nt; i++) total.sums[i] += q.sums[i];
            for (size_t i = 0; i < size_t(nout); i++) total.term[i] += q.term[i];   // one strip owns the outlet, the others say 0
        }
        float ta = 0.f;
        for (size_t i = 0; i < size_t(nout); i++) ta += total.term[i];   // file order (src/DropAnalysis.cpp:313-329)
        total_area = ta * dxA * dyA;
    }
    std::vector<float> f(4 * nt);
    for (size_t i = 0; i < nt; i++)
        for (size_t k = 0; k < 4; k++) f[k * nt + i] = float(total.sums[4 * i + k]);
    const dropan::Sums sm{int64_t(nt), total.thresh.data(), total.n1.data(), total.n2.data(), f.data(), f.data() + nt, f.data() + 2 * nt, f.data() + 3 * nt, total.length.data(),
                          total_area};
    std::string table, console;
    float opt = 0.f;
    int found = 0;
    dropan::table(sm, &table, &console, &opt, &found);
    FILE* fp = fopen(dropfile, "w");
    if (!fp) { printf("Error opening file %s.\n", dropfile); fflush(stdout); return TDX_ERR_FILE; }
    fwrite(table.data(), 1, table.size(), fp);
    fclose(fp);
    fputs(console.c_str(), stdout);
    if (threshopt) *threshopt = opt;
    return t.finish("Processes", "dropanalysis", Footer::NoWrite);
}

// The output takes the input's georeferencing and the reference's nodata tag -2 (src/PeukerDouglas.cpp:101,215), a value the tool never writes.
int tdx_tool_peukerdouglas(const char* felfile, const char* ssfile, const float* p) {
    if (!felfile || !ssfile || !p) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_peukerdouglas: bad argument");
    ToolRun t("PeukerDouglas");
    Raster fel;
    t.input(felfile, F32, fel);
    if (t.rc == TDX_OK) {   // src/PeukerDouglas.cpp:74-80
        const float timeestimate = (1e-7 * fel.info.nx * fel.info.ny / pow((double)tool_gpus(), 1)) / 60 + 1;
        fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
        fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the "
                        "computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
        fflush(stderr);
    }
    if (!t.read_done()) return t.rc;
    std::vector<int16_t> ss(t.cells());
    const float nd = (float)fel.info.nodata, p0 = p[0], p1 = p[1], p2 = p[2];
    const bool ok = t.compute([&](tdx_context* c, tdx_stats* s) { return tdx_peukerdouglas(c, fel.f.data(), fel.info.nx, fel.info.ny, nd, p0, p1, p2, ss.data(), nullptr, s); },
                              [&](RankJob& j, tdx_stats* s) {
                                  float* d_fel = j.in(fel.f);
                                  int16_t* d_ss = j.out(ss);
                                  if (j.error) return j.error;
                                  return tdx_peukerdouglas_strip(j.ctx, j.comm, d_fel, j.nx, j.nyl, nd, p0, p1, p2, d_ss, nullptr, s);
                              });
    if (!ok) return t.rc;
    t.output(ssfile, ss, fel, -2.0);
    return t.finish("Processors", "peukerdouglas");
}

}  // extern "C"

// ---- the outlet tools: MoveOutletsToStrm and ConnectDown write point layers (vector_layer.hpp)
namespace {

// where the rank threads of --gpus N meet; a rank that failed still comes, so that nobody waits for it
struct RankMeet {
    std::mutex m; std::condition_variable cv; int n = 1, here = 0, round = 0;
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        const int r = round;
        if (++here == n) { here = 0; round++; cv.notify_all(); } else cv.wait(lk, [&] { return round != r; });
    }
};

// the state of the points that walk down p, handed from strip to strip: every rank advances a copy of its own, rank 0 takes every point from the
// rank that owned its row before the round, until a round moves nothing
struct WalkState {
    std::vector<int32_t> x, y, dist, done, down;
    explicit WalkState(size_t n = 0) : x(n), y(n), dist(n, 0), done(n, 0), down(n, 0) {}
    size_t n() const { return x.size(); }
};
template <class Step>   // Step(RankJob&, WalkState& mine, int64_t* moved) -> int
int walk_over_strips(RankJob& j, RankMeet& meet, std::atomic<int>& failed, WalkState& shared, std::vector<WalkState>& copies, std::vector<int64_t>& moved,
                     std::atomic<int>& again, int first_error, Step step) {
    int e = first_error;
    const int64_t base = j.ny / j.size;
    for (;;) {
        WalkState& mine = copies[size_t(j.rank)];
        mine = shared;
        moved[size_t(j.rank)] = 0;
        if (e == TDX_OK && failed == 0) e = step(j, mine, &moved[size_t(j.rank)]);
        if (e != TDX_OK) failed = e;
        meet.wait();
        if (j.rank == 0) {
            int64_t total = 0;
            for (size_t i = 0; i < shared.n(); i++) {
                if (shared.done[i]) continue;
                const int64_t yy = shared.y[i];
                const int k = (yy < 0 || yy >= j.ny) ? 0 : int(std::min<int64_t>(yy / base, j.size - 1));
                const WalkState& c = copies[size_t(k)];
                shared.x[i] = c.x[i]; shared.y[i] = c.y[i]; shared.dist[i] = c.dist[i]; shared.done[i] = c.done[i]; shared.down[i] = c.down[i];
            }
            for (int64_t mv : moved) total += mv;
            again = (failed == 0 && total > 0) ? 1 : 0;
        }
        meet.wait();
        if (!again) break;
    }
    return e != TDX_OK ? e : int(failed);
}

int refuse_layer(const char* tool, const char* path) {
    fprintf(stderr, "taudem_amd: %s cannot write %s: %s\n", tool, path, tdx::kLayerKindsMessage);
    g_tdx_thread_error = std::string(tool) + ": unsupported output " + path;
    return TDX_ERR_ARG;
}

}  // namespace

extern "C" {

int tdx_points_write(const char* path, const double* x, const double* y, int64_t n, int32_t nfields, const char* const* names, const int32_t* types,
                     const void* const* columns) {
    if (!path || n < 0 || nfields < 0 || (n > 0 && (!x || !y)) || (nfields > 0 && (!names || !types || !columns)))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_points_write: bad argument");
    if (tdx::layer_kind(path) == tdx::LayerKind::None) return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_points_write: unsupported output ") + path + ": " + tdx::kLayerKindsMessage);
    tdx::PointLayer L;
    for (int32_t k = 0; k < nfields; k++) {
        if (!names[k] || types[k] < 0 || types[k] > 2 || (n > 0 && !columns[k])) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_points_write: bad argument");
        L.add_field(names[k], types[k] == 0 ? tdx::FieldType::Integer : types[k] == 1 ? tdx::FieldType::Real : tdx::FieldType::String);
    }
    L.resize(size_t(n));
    for (int64_t i = 0; i < n; i++) {
        L.x[size_t(i)] = x[i]; L.y[size_t(i)] = y[i];
        for (int32_t k = 0; k < nfields; k++) {
            if (types[k] == 0) L.set(size_t(i), size_t(k), (long long)static_cast<const int32_t*>(columns[k])[i]);
            else if (types[k] == 1) L.set(size_t(i), size_t(k), static_cast<const double*>(columns[k])[i]);
            else { const char* s = static_cast<const char* const*>(columns[k])[i]; L.set(size_t(i), size_t(k), std::string(s ? s : "")); }
        }
    }
    std::string err;
    if (!tdx::write_point_layer(path, L, err)) return tdx_fail(nullptr, TDX_ERR_FILE, err);
    return TDX_OK;
}

// MoveOutletsToStrm (src/MoveOutletsToStrm.cpp:80-914): reads src, then p (its words and its abort code 4 where they do not match), then the outlets
// with all their fields.  The layer arguments are accepted and ignored, as for the other outlet tools.
int tdx_tool_moveoutletstostrm(const char* pfile, const char* srcfile, const char* outletsdatasrc, const char* /*outletslayer*/, int /*uselyrname*/, int /*lyrno*/,
                               const char* outletmoveddatasrc, const char* /*outletmovedlayer*/, int maxdist) {
    if (!pfile || !srcfile || !outletsdatasrc || !outletmoveddatasrc) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_moveoutletstostrm: bad argument");
    if (tdx::layer_kind(outletmoveddatasrc) == tdx::LayerKind::None) return refuse_layer("moveoutletstostrm", outletmoveddatasrc);
    ToolRun t("MoveOutletsToStreams");
    Raster src, p;
    t.input(srcfile, I16, src);
    if (t.rc == TDX_OK) {   // :108-114
        const float timeestimate = float((2e-7 * double(src.info.nx) * double(src.info.ny) / pow(double(tool_gpus()), 0.65)) / 60 + 1);
        fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
        fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
        fflush(stderr);
    }
    t.input(pfile, I16, p, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("src and p files not the same size. Exiting \n"); fflush(stdout); return 4; }
    if (t.rc != TDX_OK) return t.rc;
    std::vector<double> ox, oy; std::vector<int> oid; std::string err;
    tdx::PointLayer layer;
    if (!tdx::read_outlets(outletsdatasrc, ox, oy, oid, err) || !tdx::read_point_fields(outletsdatasrc, ox.size(), layer, err)) {
        printf("Error Opening datasource %s.\n", outletsdatasrc);   // :186-187, exit(1)
        fflush(stdout);
        g_tdx_thread_error = err;
        return 1;
    }
    if (!t.read_done()) return t.rc;
    const size_t n = ox.size();
    if (n == 0) { printf("Unable to read any points from shapefile\n\n"); fflush(stdout); return 0; }   // :291-297; the reference runs on into empty arrays
    const int64_t nx = src.info.nx, ny = src.info.ny;
    WalkState st(n);
    for (size_t i = 0; i < n; i++) {
        int gx, gy;
        tdx::geo_to_global_xy(ox[i], oy[i], p.info.xleftedge, p.info.ytopedge, p.info.dlon, p.info.dlat, gx, gy);
        st.x[i] = gx; st.y[i] = gy;
    }
    std::vector<int32_t> src32(src.s.begin(), src.s.end()), rx(n), ry(n), rd(n);
    const int16_t p_nd = (int16_t)p.info.nodata;
    const int32_t src_nd = (int32_t)(int16_t)src.info.nodata;
    const int nranks = int(std::max<int64_t>(1, std::min<int64_t>(tool_gpus(), ny)));
    RankMeet meet; meet.n = nranks;
    std::atomic<int> failed{0}, again{0};
    std::vector<WalkState> copies(static_cast<size_t>(nranks));
    std::vector<int64_t> moved(size_t(nranks), 0);
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_moveoutlets(c, p.s.data(), src32.data(), nx, ny, p_nd, src_nd, maxdist, st.x.data(), st.y.data(), int64_t(n), rx.data(), ry.data(), rd.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_s = j.in(src32);
            const int e = walk_over_strips(j, meet, failed, st, copies, moved, again, j.error, [&](RankJob& jj, WalkState& mine, int64_t* mv) {
                return tdx_moveoutlets_strip(jj.ctx, jj.comm, d_p, d_s, jj.nx, jj.nyl, jj.y0, jj.ny, p_nd, src_nd, maxdist, mine.x.data(), mine.y.data(), mine.dist.data(),
                                             mine.done.data(), int64_t(mine.n()), mv, s);
            });
            if (j.rank == 0 && e == TDX_OK) { rx = st.x; ry = st.y; rd = st.dist; }
            return e;
        });
    if (!ok) return t.rc;
    layer.x.resize(n); layer.y.resize(n);
    const size_t kd = layer.add_field("Dist_moved", tdx::FieldType::Integer, 6);   // :275-277
    for (size_t i = 0; i < n; i++) {
        if (rd[i] < 0) { layer.x[i] = ox[i]; layer.y[i] = oy[i]; }   // not moved: the original coordinates (:744-748)
        else {                                                       // tiffIO::globalXYToGeo (src/tiffIO.cpp:593-597)
            layer.x[i] = p.info.xleftedge + p.info.dlon / 2. + rx[i] * p.info.dlon;
            layer.y[i] = p.info.ytopedge - p.info.dlat / 2. - ry[i] * p.info.dlat;
        }
        layer.set(i, kd, (long long)rd[i]);
    }
    if (!tdx::write_point_layer(outletmoveddatasrc, layer, err)) { printf(" warning: Failed to create feature in shapefile.\n"); fflush(stdout); g_tdx_thread_error = err; return TDX_ERR_FILE; }
    printf("Total time: %f\n", now_s() - t.begint);
    print_gpu_stats("moveoutletstostrm", t.st, nx * ny);
    return 0;
}

// ConnectDown (src/ConnectDown.cpp:79-893): reads w, p, ad8 with its words and its abort code 4 for a raster that does not match w.  Both layers carry
// the same id_down (w at the cell reached), the -o layer at the maxima and the -od layer at the cells reached (:732-751, :831-856).
int tdx_tool_connectdown(const char* pfile, const char* wfile, const char* ad8file, const char* outletdatasrc, const char* /*outletlyr*/,
                         const char* movedoutletdatasrc, const char* /*movedoutletlyr*/, int movedist) {
    if (!pfile || !wfile || !ad8file || !outletdatasrc || !movedoutletdatasrc) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_connectdown: bad argument");
    if (tdx::layer_kind(outletdatasrc) == tdx::LayerKind::None) return refuse_layer("connectdown", outletdatasrc);
    if (tdx::layer_kind(movedoutletdatasrc) == tdx::LayerKind::None) return refuse_layer("connectdown", movedoutletdatasrc);
    ToolRun t("ConnectDown");
    Raster w, p, ad8;
    t.input(wfile, I32, w);
    t.input(pfile, I16, p, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("w and p files not the same size. Exiting \n"); fflush(stdout); return 4; }
    t.input(ad8file, F32, ad8, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) { printf("ad8 and w files not the same size. Exiting \n"); fflush(stdout); return 4; }
    if (!t.read_done()) return t.rc;
    const int64_t nx = w.info.nx, ny = w.info.ny;
    const int16_t p_nd = (int16_t)p.info.nodata;
    const int32_t w_nd = (int32_t)w.info.nodata;
    tdx_connectdown_points* points = nullptr;
    const int nranks = int(std::max<int64_t>(1, std::min<int64_t>(tool_gpus(), ny)));
    RankMeet meet; meet.n = nranks;
    std::atomic<int> failed{0}, again{0};
    std::vector<tdx_connectdown_points*> parts(size_t(nranks), nullptr);
    std::vector<WalkState> copies(static_cast<size_t>(nranks));
    std::vector<int64_t> moved(size_t(nranks), 0);
    WalkState st;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_connectdown(c, p.s.data(), w.l.data(), ad8.f.data(), nx, ny, p_nd, w_nd, movedist, &points, s); },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            int32_t* d_w = j.in(w.l);
            float* d_a = j.in(ad8.f);
            int e = j.error;
            if (e == TDX_OK) e = tdx_connectdown_strip(j.ctx, j.comm, d_w, d_a, j.nx, j.nyl, j.y0, w_nd, &parts[size_t(j.rank)], s);
            if (e != TDX_OK) failed = e;
            meet.wait();
            if (failed == 0 && j.rank == 0) {
                const int em = tdx_connectdown_merge(parts.data(), j.size, &points);
                if (em != TDX_OK) failed = em;
                else {
                    const size_t np = size_t(tdx_connectdown_points_count(points));
                    st = WalkState(np);
                    tdx_connectdown_points_copy(points, nullptr, st.x.data(), st.y.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
                }
            }
            meet.wait();
            e = walk_over_strips(j, meet, failed, st, copies, moved, again, e, [&](RankJob& jj, WalkState& mine, int64_t* mv) {
                return tdx_connectdown_walk_strip(jj.ctx, jj.comm, d_p, d_w, jj.nx, jj.nyl, jj.y0, jj.ny, movedist, mine.x.data(), mine.y.data(), mine.dist.data(),
                                                  mine.done.data(), mine.down.data(), int64_t(mine.n()), mv, s);
            });
            if (j.rank == 0 && e == TDX_OK) e = tdx_connectdown_points_set_moved(points, st.x.data(), st.y.data(), st.down.data());
            return e;
        });
    for (tdx_connectdown_points* part : parts) tdx_connectdown_points_free(part);
    if (!ok) { tdx_connectdown_points_free(points); return t.rc; }
    const size_t np = size_t(tdx_connectdown_points_count(points));
    if (np == 0) {   // :345-351: the reference says so and runs on after MPI_Finalize; nothing is written here
        tdx_connectdown_points_free(points);
        printf("No points found\n\n");
        fflush(stdout);
        return 0;
    }
    std::vector<int32_t> ids(np), x(np), y(np), mx(np), my(np), down(np);
    std::vector<float> amax(np);
    tdx_connectdown_points_copy(points, ids.data(), x.data(), y.data(), amax.data(), mx.data(), my.data(), down.data(), nullptr);
    tdx_connectdown_points_free(points);
    std::string err;
    for (int moved_layer = 0; moved_layer < 2; moved_layer++) {
        tdx::PointLayer layer;
        const size_t ki = layer.add_field("id", tdx::FieldType::Integer), kd = layer.add_field("id_down", tdx::FieldType::Integer), ka = layer.add_field("ad8", tdx::FieldType::Real);
        layer.resize(np);
        for (size_t i = 0; i < np; i++) {   // wIO.globalXYToGeo for the maxima, p.globalXYToGeo for the cells reached: the same expression on rasters that match
            const tdx::RasterInfo& ri = moved_layer ? p.info : w.info;
            layer.x[i] = ri.xleftedge + ri.dlon / 2. + (moved_layer ? mx[i] : x[i]) * ri.dlon;
            layer.y[i] = ri.ytopedge - ri.dlat / 2. - (moved_layer ? my[i] : y[i]) * ri.dlat;
            layer.set(i, ki, (long long)ids[i]);
            layer.set(i, kd, (long long)down[i]);
            layer.set(i, ka, (double)amax[i]);
        }
        const char* path = moved_layer ? movedoutletdatasrc : outletdatasrc;
        if (!tdx::write_point_layer(path, layer, err)) { printf(" warning: Failed to create feature in shapefile.\n"); fflush(stdout); g_tdx_thread_error = err; return TDX_ERR_FILE; }
    }
    printf("Total time: %f\n", now_s() - t.begint);
    print_gpu_stats("connectdown", t.st, nx * ny);
    return 0;
}

int tdx_sinmap_read_calpar(const char* path, int32_t capacity, int32_t* reg_id, float* tmin, float* tmax, float* cmin, float* cmax, float* phimin, float* phimax,
                           float* rhos, int32_t* count) {
    if (!path || !count || capacity < 0 || (capacity > 0 && !(reg_id && tmin && tmax && cmin && cmax && phimin && phimax && rhos)))
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_sinmap_read_calpar: bad argument");
    sinmap::Regions r;
    std::string err;
    const int rc = sinmap::read_calpar(path, r, err);
    if (rc != 0) return tdx_fail(nullptr, rc == 15 ? 15 : TDX_ERR_ARG, "tdx_sinmap_read_calpar: " + err);
    *count = int32_t(r.size());
    for (size_t k = 0; k < r.size() && k < size_t(capacity); k++) {
        reg_id[k] = r.id[k];
        tmin[k] = r.tmin[k]; tmax[k] = r.tmax[k]; cmin[k] = r.cmin[k]; cmax[k] = r.cmax[k];
        phimin[k] = r.phimin[k]; phimax[k] = r.phimax[k]; rhos[k] = r.rhos[k];
    }
    return TDX_OK;
}

// The reference reads the region table before it opens a raster (an unreadable file: 15 at once), compares every raster with the slope file and
// returns 1 with a sentence naming the two files on stderr; both outputs take the slope file's georeferencing and the nodata tag -1.
int tdx_tool_sinmapsi(const char* slopefile, const char* scaterrainfile, const char* scarminroadfile, const char* scarmaxroadfile, const char* tergridfile,
                      const char* terparfile, const char* satfile, const char* sincombinedfile, double rminter, double rmaxter, const double* par) {
    if (!slopefile || !scaterrainfile || !tergridfile || !terparfile || !satfile || !sincombinedfile || !par) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_sinmapsi: bad argument");
    ToolRun t("SinmapSI");
    const float g = float(par[0]), rw = float(par[1]);   // src/SinmapSI.cpp:174-175
    sinmap::Regions reg;
    {
        std::string err;
        const int rc = sinmap::read_calpar(terparfile, reg, err);
        if (rc == 15) return 15;
        if (rc != 0) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_sinmapsi: " + err);
        if (reg.size() > 32767) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_sinmapsi: more than 32767 regions");
    }
    const bool have_min = scarminroadfile && *scarminroadfile, have_max = scarmaxroadfile && *scarmaxroadfile;
    Raster slp, sca, smin, smax, cal;
    t.input(slopefile, F32, slp);
    if (t.rc == TDX_OK) {   // src/SinmapSI.cpp:233-239
        const float timeestimate = (1e-7 * slp.info.nx * slp.info.ny / pow((double)tool_gpus(), 1)) / 60 + 1;
        fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
        fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the "
                        "computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
        fflush(stderr);
    }
    // (the last sentence says "road max contributing area" for the calibration grid: the reference's words)
    const struct { const char* path; bool have; tdx::DType type; Raster* r; const char* what; } ins[] = {
        {scaterrainfile, true, F32, &sca, "Contributing area"}, {scarminroadfile, have_min, F32, &smin, "road min contributing area"},
        {scarmaxroadfile, have_max, F32, &smax, "road max contributing area"}, {tergridfile, true, I16, &cal, "road max contributing area"}};
    for (const auto& in : ins) {
        if (!in.have || t.rc != TDX_OK) continue;
        t.input(in.path, in.type, *in.r, Mismatch::Silent);
        if (t.rc == TDX_ERR_MISMATCH) {
            fprintf(stderr, "Slope (%s) and %s (%s) files have different dimensions", slopefile, in.what, in.path);
            fflush(stderr);
            return 1;
        }
    }
    if (!t.read_done()) return t.rc;
    std::vector<float> si(t.cells()), sat(t.cells());
    const float nd = (float)slp.info.nodata;
    const double cal_nd = cal.info.nodata;
    const int32_t nreg = int32_t(reg.size());
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            return tdx_sinmapsi(c, slp.f.data(), sca.f.data(), have_min ? smin.f.data() : nullptr, have_max ? smax.f.data() : nullptr, cal.s.data(), slp.info.nx, slp.info.ny,
                                nd, cal_nd, nreg, reg.id.data(), reg.tmin.data(), reg.tmax.data(), reg.cmin.data(), reg.cmax.data(), reg.phimin.data(), reg.phimax.data(),
                                reg.rhos.data(), rminter, rmaxter, g, rw, si.data(), sat.data(), s);
        },
        [&](RankJob& j, tdx_stats* s) {
            const float* d_slp = j.in(slp.f);
            const float* d_sca = j.in(sca.f);
            const float* d_min = have_min ? j.in(smin.f) : nullptr;
            const float* d_max = have_max ? j.in(smax.f) : nullptr;
            const int16_t* d_cal = j.in(cal.s);
            float* d_si = j.out(si);
            float* d_sat = j.out(sat);
            if (j.error) return j.error;
            return tdx_sinmapsi_strip(j.ctx, j.comm, d_slp, d_sca, d_min, d_max, d_cal, j.nx, j.nyl, nd, cal_nd, nreg, reg.id.data(), reg.tmin.data(), reg.tmax.data(),
                                      reg.cmin.data(), reg.cmax.data(), reg.phimin.data(), reg.phimax.data(), reg.rhos.data(), rminter, rmaxter, g, rw, d_si, d_sat, s);
        });
    if (!ok) return t.rc;
    t.output(sincombinedfile, si, slp, -1.0);
    t.output(satfile, sat, slp, -1.0);
    return t.finish("Compute time", "sinmapsi", Footer::ComputeWrite);
}

}  // extern "C"

namespace {

// what rank 0 of TWI, SlopeArea, SlopeAreaRatio and LengthArea says on stderr once the first raster is open (src/TWI.cpp:67-73)
void print_time_estimate(const ToolRun& t, const Raster& first) {
    if (t.rc != TDX_OK) return;
    const float timeestimate = (1e-7 * first.info.nx * first.info.ny / pow((double)tool_gpus(), 1)) / 60 + 1;
    fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
    fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the "
                    "computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
    fflush(stderr);
}

// TWI, SlopeArea and SlopeAreaRatio: slp and sca in, one float raster out with the slope file's georeferencing and the nodata tag -1.  which: 0 twi, 1 sa, 2 sar
int terrain_index_tool(const char* banner, const char* stats_name, int which, const char* slopefile, const char* areafile, const char* outfile, float m, float n) {
    ToolRun t(banner);
    Raster slp, sca;
    t.input(slopefile, F32, slp);
    print_time_estimate(t, slp);
    t.input(areafile, F32, sca, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) return 1;
    if (!t.read_done()) return t.rc;
    std::vector<float> out(t.cells());
    const float slp_nd = (float)slp.info.nodata, sca_nd = (float)sca.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            float* o = out.data();
            return tdx_terrain_indices(c, slp.f.data(), sca.f.data(), slp.info.nx, slp.info.ny, slp_nd, sca_nd, m, n, which == 0 ? o : nullptr, which == 1 ? o : nullptr,
                                       which == 2 ? o : nullptr, s);
        },
        [&](RankJob& j, tdx_stats* s) {
            const float* d_slp = j.in(slp.f);
            const float* d_sca = j.in(sca.f);
            float* o = j.out(out);
            if (j.error) return j.error;
            return tdx_terrain_indices_strip(j.ctx, j.comm, d_slp, d_sca, j.nx, j.nyl, slp_nd, sca_nd, m, n, which == 0 ? o : nullptr, which == 1 ? o : nullptr,
                                             which == 2 ? o : nullptr, s);
        });
    if (!ok) return t.rc;
    t.output(outfile, out, slp, -1.0);
    return t.finish("Compute time", stats_name, Footer::ComputeLine);
}

}  // namespace

extern "C" {

int tdx_tool_twi(const char* slopefile, const char* areafile, const char* twifile) {
    if (!slopefile || !areafile || !twifile) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_twi: bad argument");
    return terrain_index_tool("Topographic Wetness Index", "twi", 0, slopefile, areafile, twifile, 0.0f, 0.0f);
}

int tdx_tool_slopearea(const char* slopefile, const char* scafile, const char* safile, const float* p) {
    if (!slopefile || !scafile || !safile || !p) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_slopearea: bad argument");
    return terrain_index_tool("SlopeArea", "slopearea", 1, slopefile, scafile, safile, p[0], p[1]);
}

int tdx_tool_slopearearatio(const char* slopefile, const char* areafile, const char* atanbfile) {
    if (!slopefile || !areafile || !atanbfile) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_slopearearatio: bad argument");
    return terrain_index_tool("SlopeAreaRatio", "slopearearatio", 2, slopefile, areafile, atanbfile, 0.0f, 0.0f);
}

// ad8 is read as the reference reads it (LONG_TYPE) and handed to the library as the float of that integer: the kernel's conversion gives the integer's
// float back, which is what the reference compares.  ss takes the ad8 file's georeferencing (src/LengthArea.cpp:142).
int tdx_tool_lengtharea(const char* plenfile, const char* ad8file, const char* ssfile, const float* p) {
    if (!plenfile || !ad8file || !ssfile || !p) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_lengtharea: bad argument");
    ToolRun t("LengthArea");
    Raster plen, ad8;
    t.input(plenfile, F32, plen);
    print_time_estimate(t, plen);
    t.input(ad8file, I32, ad8, Mismatch::Silent);
    if (t.rc == TDX_ERR_MISMATCH) return 1;
    if (t.rc == TDX_OK) {
        ad8.f.resize(ad8.l.size());
        for (size_t i = 0; i < ad8.l.size(); i++) ad8.f[i] = float(ad8.l[i]);
    }
    if (!t.read_done()) return t.rc;
    std::vector<int16_t> ss(t.cells());
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_lengtharea(c, plen.f.data(), ad8.f.data(), plen.info.nx, plen.info.ny, p[0], p[1], ss.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            const float* d_plen = j.in(plen.f);
            const float* d_ad8 = j.in(ad8.f);
            int16_t* d_ss = j.out(ss);
            if (j.error) return j.error;
            return tdx_lengtharea_strip(j.ctx, j.comm, d_plen, d_ad8, j.nx, j.nyl, p[0], p[1], d_ss, s);
        });
    if (!ok) return t.rc;
    t.output(ssfile, ss, ad8, -32768.0);
    return t.finish("Compute time", "lengtharea", Footer::ComputeLine);
}

// The region grid takes the gw file's georeferencing and the nodata tag MISSINGLONG; the one time the reference prints covers the whole run (src/SetRegion.cpp:88-185)
int tdx_tool_setregion(const char* fdrfile, const char* regiongwfile, const char* newfile, int32_t region_id) {
    if (!fdrfile || !regiongwfile || !newfile) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_setregion: bad argument");
    ToolRun t("SetRegion");
    Raster p, gw;
    t.input(fdrfile, I16, p);
    if (t.rc == TDX_OK) { fprintf(stderr, "Time estimate not available.\n"); fflush(stderr); }
    t.input(regiongwfile, I32, gw);   // "File sizes do not match" and 5 (src/SetRegion.cpp:120-125)
    if (!t.read_done()) return t.rc;
    std::vector<int32_t> out(t.cells());
    const int16_t pnd = (int16_t)p.info.nodata;
    const int32_t gnd = (int32_t)gw.info.nodata;
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_setregion(c, p.s.data(), gw.l.data(), p.info.nx, p.info.ny, pnd, gnd, region_id, out.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_p = j.in(p.s);
            const int32_t* d_gw = j.in(gw.l);
            int32_t* d_out = j.out(out);
            if (j.error) return j.error;
            return tdx_setregion_strip(j.ctx, j.comm, d_p, d_gw, j.nx, j.nyl, pnd, gnd, region_id, d_out, s);
        });
    if (!ok) return t.rc;
    t.output(newfile, out, gw, -2147483647.0);
    return t.finish("Compute time", "setregion", Footer::ComputeOnly);
}

}  // extern "C"

extern "C" {

int tdx_editraster_read_changes(const char* path, int64_t capacity, double* x, double* y, int32_t* vals, int64_t* n) {
    if (!path || !n || capacity < 0 || (capacity > 0 && (!x || !y || !vals))) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_editraster_read_changes: bad argument");
    std::vector<tdx::RasterChange> ch;
    const int rc = tdx::read_raster_changes(path, ch);
    *n = int64_t(ch.size());
    if (rc == tdx::CHANGES_NO_FILE) return tdx_fail(nullptr, TDX_ERR_FILE, std::string("tdx_editraster_read_changes: cannot open ") + path);
    for (int64_t k = 0; k < std::min<int64_t>(*n, capacity); k++) { x[k] = ch[size_t(k)].x; y[k] = ch[size_t(k)].y; vals[k] = ch[size_t(k)].val; }
    if (rc == tdx::CHANGES_RANGE)
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_editraster_read_changes: record " + std::to_string(*n) + " of " + path + " holds a value outside -32768 .. 32767");
    return TDX_OK;
}

// The change file is read once the raster is: the reference opens it after its copy pass (src/EditRaster.cpp:124) and prints one line per change it applies
// while it applies them; here the lines come before the compute step, in the same place of the output.  A change file that cannot be opened ends the
// reference in a null FILE*; a value no short holds overwrites its stack: both are refused, with nothing written.
int tdx_tool_editraster(const char* rasterfile, const char* newfile, const char* changefile) {
    if (!rasterfile || !newfile || !changefile) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_editraster: bad argument");
    ToolRun t("Editraster");
    Raster in;
    t.input(rasterfile, I16, in);
    if (t.rc == TDX_OK) { fprintf(stderr, "Time estimate not available.\n"); fflush(stderr); }
    if (!t.read_done()) return t.rc;
    const int16_t nd = (int16_t)in.info.nodata;
    std::vector<tdx::RasterChange> ch;
    const int crc = tdx::read_raster_changes(changefile, ch);
    if (crc == tdx::CHANGES_NO_FILE) {
        printf("Error opening file %s.\n", changefile);
        fflush(stdout);
        return tdx_fail(nullptr, TDX_ERR_FILE, std::string("tdx_tool_editraster: cannot open ") + changefile);
    }
    if (crc == tdx::CHANGES_RANGE) {
        fprintf(stderr, "taudem_amd: record %zu of %s holds a value outside -32768 .. 32767\n", ch.size(), changefile);
        return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_tool_editraster: a value outside -32768 .. 32767 in ") + changefile);
    }
    std::vector<int32_t> cols, rows, vals;
    for (const tdx::RasterChange& c : ch) {
        int gx, gy;
        tdx::geo_to_global_xy(c.x, c.y, in.info.xleftedge, in.info.ytopedge, in.info.dlon, in.info.dlat, gx, gy);
        if (gx < 0 || gx >= in.info.nx || gy < 0 || gy >= in.info.ny) continue;   // rasterData->isInPartition
        printf("Process: %d changing %lf, %lf, %d\n", 0, c.x, c.y, c.val);
        cols.push_back(gx); rows.push_back(gy); vals.push_back(c.val);
    }
    fflush(stdout);
    std::vector<int16_t> out(t.cells());
    const int64_t n = int64_t(cols.size());
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return tdx_editraster(c, in.s.data(), in.info.nx, in.info.ny, nd, cols.data(), rows.data(), vals.data(), n, out.data(), s); },
        [&](RankJob& j, tdx_stats* s) {
            const int16_t* d_in = j.in(in.s);
            int16_t* d_out = j.out(out);
            if (j.error) return j.error;
            return tdx_editraster_strip(j.ctx, j.comm, d_in, j.nx, j.nyl, j.y0, nd, cols.data(), rows.data(), vals.data(), n, d_out, s);
        });
    if (!ok) return t.rc;
    t.output(newfile, out, in, -32768.0);
    return t.finish("Compute time", "editraster", Footer::ComputeLine);
}

// CatchOutlets is host code from end to end: no context is created and no GPU touched.  Of p the header is read here (for the reference's words about
// it) and one cell per outlet link in tdx_catchoutlets; the reference reads the whole raster.  It prints no times (src/CatchOutlets.cpp:126-443).
int tdx_tool_catchoutlets(const char* pfile, const char* streamnetsrc, const char* treefile, const char* coordfile, const char* outletsdatasrc, double mindist,
                          int gwstartno, double minarea) {
    if (!pfile || !outletsdatasrc) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_catchoutlets: bad argument");
    const bool net = streamnetsrc && *streamnetsrc, tree = treefile && *treefile, coord = coordfile && *coordfile;
    if (net == (tree || coord) || tree != coord) {
        fprintf(stderr, "taudem_amd: catchoutlets takes the stream network either as -net <line layer> or as -tree <file> -coord <file>\n");
        return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_catchoutlets: give -net, or -tree and -coord");
    }
    if (tdx::layer_kind(outletsdatasrc) == tdx::LayerKind::None) return refuse_layer("catchoutlets", outletsdatasrc);
    if (net && tdx::layer_kind(streamnetsrc) == tdx::LayerKind::None) {
        fprintf(stderr, "taudem_amd: catchoutlets cannot read %s: %s\n", streamnetsrc, tdx::kLineLayerKindsMessage);
        return tdx_fail(nullptr, TDX_ERR_ARG, std::string("catchoutlets: unsupported input ") + streamnetsrc);
    }
    printf("Catchment Outlets version %s\n", TDVERSION);
    fflush(stdout);
    // tiffIO p(pfile, SHORT_TYPE), the time estimate and CreateNewPartition (:146-165)
    tdx::TiffReader rd;
    if (!rd.open(pfile)) { printf("Error opening file %s.\n", pfile); fflush(stdout); return tdx_fail(nullptr, TDX_ERR_FILE, rd.error()); }
    const tdx::RasterInfo& ri = rd.info();
    printf("Input file %s has %s coordinate system.\n", pfile, ri.geographic ? "geographic" : "projected");
    const float timeestimate = float((2e-7 * double(ri.nx) * double(ri.ny) / pow(1.0, 0.65)) / 60 + 1);
    fprintf(stderr, "This run may take on the order of %.0f minutes to complete.\n", timeestimate);
    fprintf(stderr, "This estimate is very approximate. \nRun time is highly uncertain as it depends on the complexity of the input data \nand speed and memory of the computer. This estimate is based on our testing on \na dual quad core Dell Xeon E5405 2.0GHz PC with 16GB RAM.\n");
    fflush(stderr);
    printf("Nodata value input to create partition from file: %lf\nNodata value recast to int16_t used in partition raster: %d\n", ri.nodata, (int16_t)ri.nodata);
    fflush(stdout);
    std::vector<tdx::NetLink> links;
    std::string err;
    if (net) {
        tdx::LineLayer L;
        if (!tdx::read_line_layer(streamnetsrc, L, err)) { printf("Error opening file %s.\n", streamnetsrc); fflush(stdout); return tdx_fail(nullptr, TDX_ERR_FILE, err); }
        if (!tdx::links_from_layer(L, links, err)) { fprintf(stderr, "taudem_amd: %s: %s\n", streamnetsrc, err.c_str()); return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_catchoutlets: " + err); }
    } else if (!tdx::links_from_text(treefile, coordfile, links, err)) {
        const bool missing = err.rfind("cannot open", 0) == 0;
        if (missing) { printf("Error opening file %s.\n", err.substr(12).c_str()); fflush(stdout); }
        else fprintf(stderr, "taudem_amd: %s\n", err.c_str());
        return tdx_fail(nullptr, missing ? TDX_ERR_FILE : TDX_ERR_ARG, "tdx_tool_catchoutlets: " + err);
    }
    tdx::FlowGrid g;
    g.nx = ri.nx; g.ny = ri.ny; g.xleftedge = ri.xleftedge; g.ytopedge = ri.ytopedge; g.dlon = ri.dlon; g.dlat = ri.dlat;
    g.p_at = [&](int64_t col, int64_t row, int16_t& dir) { return rd.read_window(col, row, 1, 1, I16, &dir); };
    std::vector<tdx::CatchOutlet> outs;
    if (!tdx::catch_outlets(links, g, mindist, gwstartno, minarea, outs, err)) {
        const bool io = err.rfind("cannot read", 0) == 0;
        if (io) { printf("Error opening file %s.\n", pfile); fflush(stdout); err += ": " + rd.error(); }
        else fprintf(stderr, "taudem_amd: %s\n", err.c_str());
        return tdx_fail(nullptr, io ? TDX_ERR_FILE : TDX_ERR_ARG, "tdx_tool_catchoutlets: " + err);
    }
    tdx::PointLayer P;
    tdx::catch_outlets_layer(links, outs, P);
    if (!tdx::write_point_layer(outletsdatasrc, P, err)) { printf("Error opening file %s.\n", outletsdatasrc); fflush(stdout); return tdx_fail(nullptr, TDX_ERR_FILE, err); }
    return 0;
}

// Watershed Grid To Shapefile (pyfiles/WatershedGridToShapefile.py: arcpy.RasterToPolygon_conversion(w, shp, "NO_SIMPLIFY", "Value")).  With --gpus N
// every rank uploads its rows WITH the neighbouring strips' rows as halo rows (the host holds the whole raster: no exchange), takes the edges of its
// owned rows, and rank 0 closes the rings over the parts in strip order: on the host, or after tdx_tool_set_polygon_rings(1) on its device.
int tdx_tool_watershedgridtoshp(const char* wfile, const char* polyfile) {
    if (!wfile || !polyfile) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_watershedgridtoshp: bad argument");
    if (tdx::layer_kind(polyfile) == tdx::LayerKind::None) return refuse_layer("watershedgridtoshp", polyfile);
    ToolRun t("WatershedGridToShapefile");
    Raster w;
    t.input(wfile, I32, w);
    if (t.rc == TDX_OK) { fprintf(stderr, "Time estimate not available.\n"); fflush(stderr); }
    if (!t.read_done()) return t.rc;
    const int64_t nx = w.info.nx, ny = w.info.ny;
    const int32_t w_nd = (int32_t)w.info.nodata;
    tdx_polygons* polys = nullptr;
    const bool device_rings = g_tool_polygon_rings == 1;
    const int nranks = int(std::max<int64_t>(1, std::min<int64_t>(tool_gpus(), ny)));
    RankMeet meet; meet.n = nranks;
    std::atomic<int> failed{0};
    std::vector<tdx_polygonize_edges*> parts(size_t(nranks), nullptr);
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) { return device_rings ? tdx_polygonize_gpu_rings(c, w.l.data(), nx, ny, w_nd, &polys, s) : tdx_polygonize(c, w.l.data(), nx, ny, w_nd, &polys, s); },
        [&](RankJob& j, tdx_stats* s) {
            int32_t* d_w = j.strip<int32_t>(nullptr);
            int e = d_w ? TDX_OK : TDX_ERR_NOMEM;
            if (e == TDX_OK) {   // rows y0 - 1 .. y1 of the raster, as far as they exist
                const int64_t r0 = std::max<int64_t>(j.y0 - 1, 0), r1 = std::min<int64_t>(j.y1 + 1, j.ny);
                if (hipMemcpyAsync(d_w + size_t(r0 - (j.y0 - 1)) * size_t(nx), w.l.data() + size_t(r0) * size_t(nx), size_t(r1 - r0) * size_t(nx) * 4, hipMemcpyHostToDevice,
                                   j.ctx->stream) != hipSuccess)
                    e = TDX_ERR_HIP;
            }
            if (e == TDX_OK) e = tdx_polygonize_edges_strip(j.ctx, j.comm, d_w, j.nx, j.nyl, j.y0, j.ny, w_nd, &parts[size_t(j.rank)], s);
            if (e != TDX_OK) failed = e;
            meet.wait();
            if (failed == 0 && j.rank == 0) {
                const int em = device_rings ? tdx_polygonize_rings_gpu(j.ctx, parts.data(), j.size, nx, ny, &polys, nullptr) : tdx_polygonize_rings(parts.data(), j.size, nx, ny, &polys);
                if (em != TDX_OK) { failed = em; e = em; }
            }
            meet.wait();
            return e != TDX_OK ? e : int(failed);
        });
    for (tdx_polygonize_edges* part : parts) tdx_polygonize_edges_free(part);
    if (!ok) { tdx_polygons_free(polys); return t.rc; }
    int64_t np = 0, nr = 0, nv = 0;
    const int64_t nf = tdx_polygons_count(polys, &np, &nr, &nv, nullptr);
    const int wrc = tdx_polygons_write(polyfile, polys, w.info.gt);
    tdx_polygons_free(polys);
    if (wrc != TDX_OK) { printf("Error opening file %s.\n", polyfile); fflush(stdout); return wrc; }
    printf("Polygons: %lld features, %lld polygons, %lld rings, %lld vertices\n", (long long)nf, (long long)np, (long long)nr, (long long)nv);
    return t.finish("Processes", "watershedgridtoshp");
}

// Create Parameter Region Grid (pyfiles/SIRegionTool.py): the calibration region grid on the DEM's grid - one region, a polygon layer burned in by an
// attribute, or an existing region grid resampled by nearest neighbour - and the region table with one line per id that occurs.  With --gpus N every
// rank computes its row strip (a resampled source is uploaded whole to every rank); the ids of the strips are united on the host.
namespace {
bool parent_exists(const std::string& path) {
    const size_t k = path.find_last_of('/');
    if (k == std::string::npos) return true;
    struct stat sb;
    const std::string dir = k == 0 ? std::string("/") : path.substr(0, k);
    return stat(dir.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode);
}
}  // namespace

int tdx_tool_siregiontool(const char* demfile, const char* parregfile, const char* attfile, const char* parreg_infile, const char* shpfile, const char* shp_att_name,
                          const char* const* seven_texts) {
    if (!demfile || !parregfile || !attfile || !seven_texts) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_siregiontool: bad argument");
    for (int k = 0; k < 7; k++)
        if (!seven_texts[k]) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_tool_siregiontool: bad argument");
    const bool have_src = parreg_infile && *parreg_infile, have_shp = shpfile && *shpfile;
    if (have_src && have_shp) return tdx_fail(nullptr, TDX_ERR_ARG, "siregiontool: a region grid and a region polygon layer were both given: give one, or neither");
    if (have_shp && tdx::layer_kind(shpfile) == tdx::LayerKind::None)
        return tdx_fail(nullptr, TDX_ERR_ARG, std::string("siregiontool: unsupported input ") + shpfile + ": " + tdx::kPolygonLayerKindsMessage);
    for (const char* out : {parregfile, attfile})
        if (!parent_exists(out)) return tdx_fail(nullptr, TDX_ERR_ARG, std::string("siregiontool: the directory of ") + out + " does not exist");
    ToolRun t("SIRegionTool");
    Raster dem, src;
    t.input(demfile, F32, dem);
    if (t.rc == TDX_OK && have_src) t.rc = load_raster(parreg_infile, I32, src);
    std::vector<double> x, y;
    std::vector<int64_t> ring_first{0}, feature_first{0};
    std::vector<int32_t> values;
    if (t.rc == TDX_OK && have_shp) {
        tdx::PolygonLayer L;
        std::string err;
        if (!tdx::read_polygon_layer(shpfile, L, err)) return tdx_fail(nullptr, TDX_ERR_FILE, "siregiontool: " + err);
        if (!regions::attribute_values(L, shp_att_name && *shp_att_name ? shp_att_name : "ID", values, err)) return tdx_fail(nullptr, TDX_ERR_ARG, "siregiontool: " + err);
        for (const auto& feat : L.polygons) {
            for (const auto& pg : feat)
                for (const auto& rg : pg) {
                    x.insert(x.end(), rg.x.begin(), rg.x.end());
                    y.insert(y.end(), rg.y.begin(), rg.y.end());
                    ring_first.push_back(int64_t(x.size()));
                }
            feature_first.push_back(int64_t(ring_first.size()) - 1);
        }
    }
    if (!t.read_done()) return t.rc;
    const int64_t nx = dem.info.nx, ny = dem.info.ny;
    const double* gt = dem.info.gt;
    const int64_t n_rings = int64_t(ring_first.size()) - 1, n_features = int64_t(values.size());
    const int32_t src_nd = have_src ? (int32_t)src.info.nodata : 0;
    std::vector<int16_t> out(t.cells());
    const int nranks = int(std::max<int64_t>(1, std::min<int64_t>(tool_gpus(), ny)));
    std::vector<std::vector<int32_t>> ids(size_t(nranks), std::vector<int32_t>(TDX_REGIONGRID_MAX_IDS));
    std::vector<int32_t> n_ids(size_t(nranks), 0);
    const bool ok = t.compute(
        [&](tdx_context* c, tdx_stats* s) {
            if (have_shp)
                return tdx_regiongrid(c, x.data(), y.data(), ring_first.data(), n_rings, feature_first.data(), values.data(), n_features, gt, 0, nx, ny, out.data(),
                                      ids[0].data(), &n_ids[0], nullptr, nullptr, s);
            if (have_src)
                return tdx_regiongrid_resample(c, src.l.data(), src.info.nx, src.info.ny, src.info.gt, src_nd, gt, nx, ny, out.data(), ids[0].data(), &n_ids[0], nullptr, s);
            return tdx_regiongrid_constant(c, nx, ny, out.data(), ids[0].data(), &n_ids[0], s);
        },
        [&](RankJob& j, tdx_stats* s) {
            int16_t* d_out = j.out(out);
            if (j.error) return j.error;
            const size_t r = size_t(j.rank);
            if (have_shp)
                return tdx_regiongrid_strip(j.ctx, j.comm, x.data(), y.data(), ring_first.data(), n_rings, feature_first.data(), values.data(), n_features, gt, 0, j.nx,
                                            j.nyl, j.y0, j.ny, d_out, ids[r].data(), &n_ids[r], nullptr, nullptr, s);
            if (have_src) {
                void* d_src = nullptr;
                const size_t bytes = src.l.size() * 4;
                if (hipMalloc(&d_src, bytes) != hipSuccess) { (void)hipGetLastError(); return int(TDX_ERR_NOMEM); }
                j.owned.push_back(d_src);
                if (hipMemcpyAsync(d_src, src.l.data(), bytes, hipMemcpyHostToDevice, j.ctx->stream) != hipSuccess) return int(TDX_ERR_HIP);
                return tdx_regiongrid_resample_strip(j.ctx, j.comm, static_cast<const int32_t*>(d_src), src.info.nx, src.info.ny, src.info.gt, src_nd, gt, j.nx, j.nyl, j.y0,
                                                     j.ny, d_out, ids[r].data(), &n_ids[r], nullptr, s);
            }
            return tdx_regiongrid_constant_strip(j.ctx, j.comm, j.nx, j.nyl, j.y0, j.ny, d_out, ids[r].data(), &n_ids[r], s);
        });
    if (!ok) return t.rc;
    std::vector<int32_t> all;
    for (size_t r = 0; r < ids.size(); r++) all.insert(all.end(), ids[r].begin(), ids[r].begin() + n_ids[r]);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    t.output(parregfile, out, dem, 0.0);
    if (t.rc == TDX_OK) {
        std::string err;
        if (!regions::write_table(attfile, all.data(), int32_t(all.size()), seven_texts, err)) return tdx_fail(nullptr, TDX_ERR_FILE, "siregiontool: " + err);
    }
    printf("Regions: %lld\n", (long long)all.size());
    return t.finish("Processes", "siregiontool");
}

// ---- a polygon layer read from a file (host code, no context)
struct tdx_polygon_layer { tdx::PolygonLayer L; };

int tdx_polygon_layer_read(const char* path, tdx_polygon_layer** layer) {
    if (!path || !layer) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygon_layer_read: bad argument");
    *layer = nullptr;
    tdx_polygon_layer* res = new tdx_polygon_layer;
    std::string err;
    const bool known = tdx::layer_kind(path) != tdx::LayerKind::None;
    if (!tdx::read_polygon_layer(path, res->L, err)) { delete res; return tdx_fail(nullptr, known ? TDX_ERR_FILE : TDX_ERR_ARG, "tdx_polygon_layer_read: " + err); }
    *layer = res;
    return TDX_OK;
}
int64_t tdx_polygon_layer_count(const tdx_polygon_layer* layer, int64_t* n_rings, int64_t* n_vertices, int64_t* n_fields) {
    int64_t nr = 0, nv = 0;
    if (layer)
        for (const auto& feat : layer->L.polygons)
            for (const auto& pg : feat)
                for (const auto& rg : pg) { nr++; nv += int64_t(rg.x.size()); }
    if (n_rings) *n_rings = nr;
    if (n_vertices) *n_vertices = nv;
    if (n_fields) *n_fields = layer ? int64_t(layer->L.fields.size()) : 0;
    return layer ? int64_t(layer->L.polygons.size()) : 0;
}
void tdx_polygon_layer_copy(const tdx_polygon_layer* layer, int64_t* feature_first, int64_t* ring_first, double* x, double* y) {
    if (!layer) return;
    int64_t nr = 0, nv = 0;
    size_t f = 0;
    if (feature_first) feature_first[0] = 0;
    if (ring_first) ring_first[0] = 0;
    for (const auto& feat : layer->L.polygons) {
        for (const auto& pg : feat)
            for (const auto& rg : pg) {
                for (size_t k = 0; k < rg.x.size(); k++, nv++) { if (x) x[nv] = rg.x[k]; if (y) y[nv] = rg.y[k]; }
                nr++;
                if (ring_first) ring_first[nr] = nv;
            }
        f++;
        if (feature_first) feature_first[f] = nr;
    }
}
const char* tdx_polygon_layer_field(const tdx_polygon_layer* layer, int64_t k) {
    return layer && k >= 0 && size_t(k) < layer->L.fields.size() ? layer->L.fields[size_t(k)].name.c_str() : nullptr;
}
const char* tdx_polygon_layer_value(const tdx_polygon_layer* layer, int64_t feature, int64_t k) {
    if (!layer || feature < 0 || size_t(feature) >= layer->L.values.size() || k < 0 || size_t(k) >= layer->L.values[size_t(feature)].size()) return nullptr;
    return layer->L.values[size_t(feature)][size_t(k)].c_str();
}
int tdx_polygon_layer_values(const tdx_polygon_layer* layer, const char* field, int32_t* values) {
    if (!layer || !field) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygon_layer_values: bad argument");
    std::vector<int32_t> v;
    std::string err;
    if (!regions::attribute_values(layer->L, field, v, err)) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygon_layer_values: " + err);
    if (values && !v.empty()) memcpy(values, v.data(), v.size() * 4);
    return TDX_OK;
}
void tdx_polygon_layer_free(tdx_polygon_layer* layer) { delete layer; }

}  // extern "C"
