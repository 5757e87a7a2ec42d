// Host side of CatchHydroGeo and InunDepth (hand_tables.hpp): catchment list, stage file, forecast file and hydraulic property table in; the table and the
// depth CSV out.
#include "hand_tables.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace handtables {

namespace {
constexpr int kLine = 256;    // the reference's CSV line buffer
constexpr int kLong = 4096;   // MAXLN (src/commonLib.h)

// data lines after the header, and the file position of the first one
int count_rows(FILE* f, long& data) {
    char line[kLine];
    data = ftell(f);
    int n = 0;
    while (fgets(line, sizeof line, f))
        if (line[0] != '\n' && line[0] != '\0') n++;
    return n;
}
}  // namespace

bool read_catch_list(const char* path, CatchList& out) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "ERROR: Cannot open catch list file!\n"); return false; }
    char line[kLine];
    if (!fgets(line, sizeof line, f)) { fprintf(stderr, "ERROR: Empty catch list file!\n"); fclose(f); return false; }
    long data;
    const int n = count_rows(f, data);
    if (n <= 0) { fprintf(stderr, "ERROR: catch list empty!\n"); fclose(f); return false; }
    fseek(f, data, SEEK_SET);
    int cols = 3;
    if (fgets(line, sizeof line, f)) {   // the first data line decides
        cols = 0;
        for (char* t = strtok(line, ","); t; t = strtok(nullptr, ",")) cols++;
        fseek(f, data, SEEK_SET);
    }
    if (cols < 3) { fprintf(stderr, "ERROR: Catchment list file must have at least 3 columns (id, slope, length).\n"); fclose(f); return false; }
    const bool has_n = cols == 4;
    if (!has_n) fprintf(stderr, "INFO: Mannings n not found in catchment list file. Using default value of 0.05 for all catchments.\n");
    out.id.assign(size_t(n), 0); out.slope.assign(size_t(n), 0.0); out.length.assign(size_t(n), 0.0); out.manning.assign(size_t(n), 0.05);
    int i = 0;
    while (fgets(line, sizeof line, f) && i < n) {
        char* t = strtok(line, ",");
        if (!t) continue;
        out.id[size_t(i)] = atoi(t);
        if (!(t = strtok(nullptr, ","))) { fprintf(stderr, "ERROR: Missing slope value for catchment id %d in catchment list file.\n", out.id[size_t(i)]); fclose(f); return false; }
        out.slope[size_t(i)] = atof(t);
        if (!(t = strtok(nullptr, ","))) { fprintf(stderr, "ERROR: Missing length value for catchment id %d in catchment list file.\n", out.id[size_t(i)]); fclose(f); return false; }
        out.length[size_t(i)] = atof(t);
        if (has_n && (t = strtok(nullptr, ","))) out.manning[size_t(i)] = atof(t);
        i++;
    }
    fclose(f);
    return true;
}

bool read_stages(const char* path, std::vector<double>& stage) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char line[kLong];
    int lines = 0;
    while (fgets(line, sizeof line, f)) lines++;
    const int nh = lines - 1;   // the first line is the header
    stage.assign(size_t(nh > 0 ? nh : 0), 0.0);
    rewind(f);
    for (int ch = getc(f); ch != EOF && ch != '\n'; ch = getc(f)) {}
    for (int k = 0; k < nh; k++)
        if (fscanf(f, "%lf\n", &stage[size_t(k)]) != 1) break;
    fclose(f);
    return true;
}

bool write_hydroprop(const char* path, const CatchList& cl, const std::vector<double>& stage, const std::vector<int32_t>& count, const std::vector<double>& surface,
                     const std::vector<double>& bed, const std::vector<double>& volume, const std::vector<double>& catcharea) {
    FILE* f = fopen(path, "w");
    if (!f) return false;
    const size_t nc = cl.id.size(), nh = stage.size();
    fprintf(f, "Id, Stage_m, Number of Cells, ReachWetArea_m2, ReachBedArea_m2, ReachVolume_m3, ReachSlope, ReachLength_m, CatchArea_m2, CrossSectionalArea_m2, "
               "WetPerimeter_m, HydRadius_m, Manning_n, Flow_m3s\n");
    for (size_t c = 0; c < nc; c++)
        for (size_t k = 0; k < nh; k++) {
            const size_t t = k * nc + c;
            double section = 0.0, perimeter = 0.0, radius = 0.0, flow = 0.0;
            if (volume[t] > 0) {
                if (cl.length[c] > 0) { section = volume[t] / cl.length[c]; perimeter = bed[t] / cl.length[c]; }
                if (perimeter > 0) {
                    radius = section / perimeter;
                    flow = (section * pow(radius, 2.0 / 3.0) * sqrt(cl.slope[c])) / cl.manning[c];   // Manning
                }
            }
            fprintf(f, "%d,%.6lf,%d,%.6lf,%.6lf,%.6lf,%.10lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf\n", cl.id[c], stage[k], count[t], surface[t], bed[t], volume[t],
                    cl.slope[c], cl.length[c], catcharea[c], section, perimeter, radius, cl.manning[c], flow);
        }
    fclose(f);
    return true;
}

bool read_forecast(const char* fcfile, const char* hpfile, Forecast& out) {
    char head[kLong], line[kLine];
    FILE* f = fopen(fcfile, "r");
    if (!f) { fprintf(stderr, "Error: Cannot open forecast file %s\n", fcfile); return false; }
    if (!fgets(head, sizeof head, f)) { fprintf(stderr, "Error: Empty forecast file %s\n", fcfile); fclose(f); return false; }
    long data;
    const int nfc = count_rows(f, data);
    if (nfc <= 0) { fprintf(stderr, "Error: No data found in forecast file %s\n", fcfile); fclose(f); return false; }
    out.id.assign(size_t(nfc), 0); out.flow.assign(size_t(nfc), 0.0);
    fseek(f, data, SEEK_SET);
    for (int i = 0; i < nfc; i++) {
        int id;
        if (fscanf(f, "%d,%lf", &id, &out.flow[size_t(i)]) != 2) { fprintf(stderr, "Error: Failed to read data at line %ld in file %s\n", long(i + 2), fcfile); fclose(f); return false; }
        out.id[size_t(i)] = id;
    }
    fclose(f);

    f = fopen(hpfile, "r");
    if (!f) { fprintf(stderr, "Error: Cannot open hydroprop file %s\n", hpfile); return false; }
    if (!fgets(head, sizeof head, f)) { fprintf(stderr, "Error: Empty hydroprop file %s\n", hpfile); fclose(f); return false; }
    const int nhp = count_rows(f, data);
    if (nhp <= 0) { fprintf(stderr, "Error: No data found in hydroprop file %s\n", hpfile); fclose(f); return false; }
    std::vector<int32_t> hid(static_cast<size_t>(nhp));
    std::vector<float> hstage(static_cast<size_t>(nhp)), harea(static_cast<size_t>(nhp)), hflow(static_cast<size_t>(nhp));   // read as FLOAT, as the reference
    fseek(f, data, SEEK_SET);
    for (int r = 0; r < nhp; r++) {
        const long ln = long(r + 2);
        if (!fgets(line, sizeof line, f)) { fprintf(stderr, "Error: Failed to read line %ld in file %s\n", ln, hpfile); fclose(f); return false; }
        char* t = strtok(line, ",");
        for (int col = 1; col <= 14; col++) {
            if (!t) {
                if (col == 1) fprintf(stderr, "Error: Failed to parse ID at line %ld in file %s\n", ln, hpfile);
                else if (col == 2) fprintf(stderr, "Error: Failed to parse Stage at line %ld in file %s\n", ln, hpfile);
                else if (col == 9) fprintf(stderr, "Error: Failed to parse CatchArea at line %ld in file %s\n", ln, hpfile);
                else if (col == 14) fprintf(stderr, "Error: Failed to parse Flow at line %ld in file %s\n", ln, hpfile);
                else fprintf(stderr, "Error: Failed to parse column %d at line %ld in file %s\n", col, ln, hpfile);
                fclose(f);
                return false;
            }
            if (col == 1) hid[size_t(r)] = atoi(t);
            else if (col == 2) hstage[size_t(r)] = float(atof(t));
            else if (col == 9) harea[size_t(r)] = float(atof(t));
            else if (col == 14) hflow[size_t(r)] = float(atof(t));
            if (col < 14) t = strtok(nullptr, col == 13 ? ",\n\r" : ",");
        }
    }
    fclose(f);
    out.depth.assign(size_t(nfc), -9999.0f);
    out.catcharea.assign(size_t(nfc), -9999.0f);
    std::unordered_map<int32_t, float> area_of;   // last row wins
    for (int r = 0; r < nhp; r++) area_of[hid[size_t(r)]] = harea[size_t(r)];
    for (int i = 0; i < nfc; i++) {
        const double q = out.flow[size_t(i)];
        double q_lo = -1, q_hi = -1, h_lo = -1, h_hi = -1;
        bool lo = false, hi = false;
        for (int r = 0; r < nhp && !hi; r++) {   // rows in file order: the last row at or below q, the FIRST at or above it
            if (hid[size_t(r)] != out.id[size_t(i)]) continue;
            if (hflow[size_t(r)] <= q) { q_lo = hflow[size_t(r)]; h_lo = hstage[size_t(r)]; lo = true; }
            if (hflow[size_t(r)] >= q) { q_hi = hflow[size_t(r)]; h_hi = hstage[size_t(r)]; hi = true; }
        }
        double d = -9999.0;
        if (lo && hi && q_hi > q_lo) d = (q - q_lo) / (q_hi - q_lo) * (h_hi - h_lo) + h_lo;
        out.depth[size_t(i)] = float(d);
        const auto it = area_of.find(out.id[size_t(i)]);
        if (it != area_of.end()) out.catcharea[size_t(i)] = it->second;
    }
    return true;
}

void write_depths(const char* path, const Forecast& fc, const std::vector<float>& area) {
    FILE* f = fopen(path, "w");
    if (!f) { fprintf(stderr, "Error: Cannot create depth file %s\n", path); return; }
    fprintf(f, "id,flow,depth,InunArea_m2,CatchArea_m2,InunRatio\n");
    std::unordered_map<int32_t, size_t> win;   // last row wins
    for (size_t i = 0; i < fc.id.size(); i++) win[fc.id[i]] = i;
    const float none = -9999.0f;
    for (size_t i = 0; i < fc.id.size(); i++) {
        const size_t w = win[fc.id[i]];
        const double depth = fc.depth[w];
        const float wet = area[w] > 0 ? area[w] : none;
        const float whole = fc.catcharea[i];
        float ratio = none;
        if (wet != none && whole != none) ratio = wet / whole;
        fprintf(f, "%d,%.6f,%.6f,%.6f,%.6f,%.6f\n", fc.id[i], fc.flow[i], depth, wet, whole, ratio);
    }
    fclose(f);
}

}  // namespace handtables
