/* A plain C restatement of CatchHydroGeo (catchhydrogeo, src/CatchHydroGeo.cpp) and InunDepth (inundepth, src/InunDepth.cpp), written from
 * the rules of DESIGN.md section "CatchHydroGeo and InunDepth": one raster scan, row by row, with running sums - not the tiled two-pass
 * reduction of the GPU kernels, which it is there to check.  It also restates the host part: the three CSV readers, the stage reader, the
 * flow-to-depth interpolation and the two table writers.  Its own CPU test holds it to every golden byte for byte.  Built by the tests
 * with `cc -O2 -ffp-contract=off -shared -fPIC`.  Functions return 0, or a negative number for a file that cannot be read. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LINE 256      /* the line buffer of the CSV readers */
#define LONGLINE 4096 /* MAXLN: the buffer the stage file's lines are counted with */

/* linearpart<T>::isNodata (src/linearpart.h:476): for integers the difference is an integer, so the test is equality */
static int nodata_f(float v, float nd) { return fabsf((float)(v - nd)) < 1e-5f; }
static int nodata_i(int32_t v, int32_t nd) { return v == nd; }
static int nodata_s(int16_t v, int16_t nd) { return v == nd; }

/* an unordered_map filled in list order: the LAST entry with the id is the one found; -1: none */
static int last_index(const int32_t* ids, int n, int32_t id) {
    for (int i = n - 1; i >= 0; i--)
        if (ids[i] == id) return i;
    return -1;
}

/* ---- CatchHydroGeo ---------------------------------------------------------------------------------------------------------------- */

/* The per-cell loop (src/CatchHydroGeo.cpp:285-311).  count / surf / bed / vol: [nh][ncatch], carea: [ncatch], all zeroed here. */
int chg_sums(int nx, int ny, const float* hand, float hand_nd, const int32_t* cat, int32_t cat_nd, const float* slp, float slp_nd, const double* dxc,
             const double* dyc, const int32_t* ids, int ncatch, const double* stage, int nh, int32_t* count, double* surf, double* bed, double* vol,
             double* carea) {
    const size_t nt = (size_t)nh * (size_t)ncatch;
    memset(count, 0, nt * sizeof(int32_t));
    for (size_t t = 0; t < nt; t++) surf[t] = bed[t] = vol[t] = 0.0;
    for (int c = 0; c < ncatch; c++) carea[c] = 0.0;
    int32_t seen_id = 0;
    int seen = -2; /* the previous cell's lookup, reused while the id stays the same */
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t cell = (size_t)j * nx + i;
            if (nodata_i(cat[cell], cat_nd)) continue;
            if (seen == -2 || cat[cell] != seen_id) { seen_id = cat[cell]; seen = last_index(ids, ncatch, seen_id); }
            if (seen < 0) continue;
            const double area = dxc[j] * dyc[j];
            carea[seen] += area;
            if (nodata_f(hand[cell], hand_nd) || nodata_f(slp[cell], slp_nd)) continue;
            const float h = hand[cell], s = slp[cell];
            const float root = sqrtf(1 + s * s); /* 1 + float * float is a float, and sqrt of a float is the float overload */
            for (int k = 0; k < nh; k++) {
                if (h < stage[k] || fabs(h - 0.0) < 0.000001) {
                    const size_t t = (size_t)k * ncatch + seen;
                    count[t] += 1;
                    surf[t] += area;
                    bed[t] += area * root;
                    vol[t] += (stage[k] - h) * area;
                }
            }
        }
    return 0;
}

/* The catchment list (src/CatchHydroGeo.cpp:128-212).  *n_out rows, at most cap; returns -1 no file, -2 no header, -3 no rows, -4 fewer than
 * three columns, -5 / -6 a row without slope / length.  *four: 1 when the first data row has exactly four columns. */
int chg_read_list(const char* path, int cap, int32_t* ids, double* slope, double* length, double* mann, int* n_out, int* four) {
    FILE* f = fopen(path, "r");
    char line[LINE], copy[LINE];
    if (!f) return -1;
    if (!fgets(line, sizeof line, f)) { fclose(f); return -2; }
    const long data = ftell(f);
    int n = 0;
    while (fgets(line, sizeof line, f))
        if (line[0] != '\n' && line[0] != '\0') n++;
    if (n <= 0) { fclose(f); return -3; }
    fseek(f, data, SEEK_SET);
    int cols = 3;
    if (fgets(line, sizeof line, f)) {
        strcpy(copy, line);
        cols = 0;
        for (char* t = strtok(copy, ","); t; t = strtok(NULL, ",")) cols++;
        fseek(f, data, SEEK_SET);
    }
    if (cols < 3) { fclose(f); return -4; }
    *four = cols == 4;
    int i = 0;
    while (fgets(line, sizeof line, f) && i < n && i < cap) {
        char* t = strtok(line, ",");
        if (!t) continue;
        ids[i] = atoi(t);
        if (!(t = strtok(NULL, ","))) { fclose(f); return -5; }
        slope[i] = atof(t);
        if (!(t = strtok(NULL, ","))) { fclose(f); return -6; }
        length[i] = atof(t);
        mann[i] = 0.05;
        if (*four && (t = strtok(NULL, ","))) mann[i] = atof(t);
        i++;
    }
    fclose(f);
    *n_out = n; /* rows the file has no text for keep what the caller put there */
    return 0;
}

/* The stage file (src/CatchHydroGeo.cpp:230-252): lines counted with a 4096-byte buffer, minus the header; values with "%lf\n". */
int chg_read_stages(const char* path, int cap, double* stage, int* nh_out) {
    FILE* f = fopen(path, "r");
    char line[LONGLINE];
    if (!f) return -1;
    int lines = 0;
    while (fgets(line, sizeof line, f)) lines++;
    const int nh = lines - 1;
    rewind(f);
    int ch;
    while ((ch = getc(f)) != EOF && ch != '\n') {}
    for (int k = 0; k < nh && k < cap; k++)
        if (fscanf(f, "%lf\n", &stage[k]) != 1) break;
    fclose(f);
    *nh_out = nh;
    return 0;
}

/* Derived columns and the table (src/CatchHydroGeo.cpp:335-373) */
int chg_write_table(const char* path, const int32_t* ids, const double* slope, const double* length, const double* mann, int ncatch, const double* stage, int nh,
                    const int32_t* count, const double* surf, const double* bed, const double* vol, const double* carea) {
    FILE* f = fopen(path, "w");
    if (!f) return -1;
    fprintf(f, "Id, Stage_m, Number of Cells, ReachWetArea_m2, ReachBedArea_m2, ReachVolume_m3, ReachSlope, ReachLength_m, CatchArea_m2, CrossSectionalArea_m2, "
               "WetPerimeter_m, HydRadius_m, Manning_n, Flow_m3s\n");
    for (int c = 0; c < ncatch; c++)
        for (int k = 0; k < nh; k++) {
            const size_t t = (size_t)k * ncatch + c;
            double xs = 0.0, wp = 0.0, hr = 0.0, q = 0.0;
            if (vol[t] > 0) {
                if (length[c] > 0) { xs = vol[t] / length[c]; wp = bed[t] / length[c]; }
                if (wp > 0) { hr = xs / wp; q = (xs * pow(hr, 2.0 / 3.0) * sqrt(slope[c])) / mann[c]; }
            }
            fprintf(f, "%d,%.6lf,%d,%.6lf,%.6lf,%.6lf,%.10lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf,%.6lf\n", ids[c], stage[k], count[t], surf[t], bed[t], vol[t], slope[c],
                    length[c], carea[c], xs, wp, hr, mann[c], q);
        }
    fclose(f);
    return 0;
}

/* ---- InunDepth -------------------------------------------------------------------------------------------------------------------- */

/* Forecast file + hydraulic property table -> one depth per forecast row (src/InunDepth.cpp:111-347).  carea[i]: the CatchArea column of the
 * LAST table row with the id, -9999 without one.  Returns -1 / -2 / -3 (forecast: no file, empty, no rows), -4 a bad forecast row,
 * -5 / -6 / -7 (table: no file, empty, no rows), -8 a short table row. */
int inun_depths(const char* fcfile, const char* hpfile, int cap, int32_t* ids, double* flow, float* depth, float* carea, int* nfc_out) {
    char line[LINE], head[LONGLINE];
    FILE* f = fopen(fcfile, "r");
    if (!f) return -1;
    if (!fgets(head, sizeof head, f)) { fclose(f); return -2; }
    long data = ftell(f);
    int nfc = 0;
    while (fgets(line, sizeof line, f))
        if (line[0] != '\n' && line[0] != '\0') nfc++;
    if (nfc <= 0) { fclose(f); return -3; }
    if (nfc > cap) nfc = cap;
    fseek(f, data, SEEK_SET);
    for (int i = 0; i < nfc; i++) {
        int id;
        if (fscanf(f, "%d,%lf", &id, &flow[i]) != 2) { fclose(f); return -4; }
        ids[i] = id;
    }
    fclose(f);

    f = fopen(hpfile, "r");
    if (!f) return -5;
    if (!fgets(head, sizeof head, f)) { fclose(f); return -6; }
    data = ftell(f);
    int nhp = 0;
    while (fgets(line, sizeof line, f))
        if (line[0] != '\n' && line[0] != '\0') nhp++;
    if (nhp <= 0) { fclose(f); return -7; }
    int32_t* hid = malloc(sizeof(int32_t) * (size_t)nhp);
    float* hstage = malloc(sizeof(float) * (size_t)nhp);
    float* harea = malloc(sizeof(float) * (size_t)nhp);
    float* hflow = malloc(sizeof(float) * (size_t)nhp);
    fseek(f, data, SEEK_SET);
    int bad = 0;
    for (int r = 0; r < nhp && !bad; r++) {
        if (!fgets(line, sizeof line, f)) { bad = 1; break; }
        char* t = strtok(line, ",");
        for (int col = 1; col <= 14; col++) {
            if (!t) { bad = 1; break; }
            if (col == 1) hid[r] = atoi(t);
            else if (col == 2) hstage[r] = atof(t);
            else if (col == 9) harea[r] = atof(t);
            else if (col == 14) hflow[r] = atof(t);
            if (col < 14) t = strtok(NULL, col == 13 ? ",\n\r" : ",");
        }
    }
    fclose(f);
    if (!bad) {
        for (int i = 0; i < nfc; i++) {
            double q1 = -1, q2 = -1, h1 = -1, h2 = -1, d = -9999.0;
            int lower = 0, upper = 0;
            for (int r = 0; r < nhp; r++) {
                if (hid[r] != ids[i]) continue;
                if (hflow[r] <= flow[i]) { q1 = hflow[r]; h1 = hstage[r]; lower = 1; }
                if (hflow[r] >= flow[i]) { q2 = hflow[r]; h2 = hstage[r]; upper = 1; break; }
            }
            if (lower && upper && q2 > q1) d = (flow[i] - q1) / (q2 - q1) * (h2 - h1) + h1;
            depth[i] = d;
            carea[i] = -9999.0f;
            for (int r = nhp - 1; r >= 0; r--)
                if (hid[r] == ids[i]) { carea[i] = harea[r]; break; }
        }
    }
    free(hid); free(hstage); free(harea); free(hflow);
    *nfc_out = nfc;
    return bad ? -8 : 0;
}

/* The depth raster (src/InunDepth.cpp:449-473), nodata -3.0e38f.  mask == NULL: no -mask.  With a mask every cell stays nodata: at the
 * reference's line 465 the id has always been found already. */
int inun_map(int nx, int ny, const float* hand, float hand_nd, const int32_t* cat, int32_t cat_nd, const int16_t* mask, int16_t mask_nd, const int32_t* ids,
             const float* depth, int nfc, float* map) {
    const float none = -3.0e38;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t cell = (size_t)j * nx + i;
            map[cell] = none;
            if (nodata_i(cat[cell], cat_nd) || nodata_f(hand[cell], hand_nd)) continue;
            if (mask && !nodata_s(mask[cell], mask_nd)) continue;
            const int at = last_index(ids, nfc, cat[cell]);
            if (at < 0) continue;
            const double hfc = depth[at];
            if (hfc < 0.0) continue;
            if (mask) continue;
            const float hv = hand[cell];
            if (hfc > hv + 0.001) map[cell] = (float)(hfc - (double)hv);
        }
    return 0;
}

/* Inundated area per forecast row (src/InunDepth.cpp:366-412): a running FLOAT sum, at the last row with the id */
int inun_area(int nx, int ny, const float* hand, float hand_nd, const int32_t* cat, int32_t cat_nd, const double* dxc, const double* dyc, const int32_t* ids,
              const float* depth, int nfc, float* area) {
    for (int i = 0; i < nfc; i++) area[i] = 0.0f;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t cell = (size_t)j * nx + i;
            if (nodata_i(cat[cell], cat_nd) || nodata_f(hand[cell], hand_nd)) continue;
            const int at = last_index(ids, nfc, cat[cell]);
            if (at < 0) continue;
            const float d = depth[at];
            if (!(d > 0)) continue;
            const double a = dxc[j] * dyc[j];
            if ((d - hand[cell]) > 0.0) area[at] += a;
        }
    return 0;
}

/* The depth CSV (src/InunDepth.cpp:416-442); area as inun_area() gives it */
int inun_write_depths(const char* path, const int32_t* ids, const double* flow, const float* depth, const float* area, const float* carea, int nfc) {
    FILE* f = fopen(path, "w");
    if (!f) return -1;
    fprintf(f, "id,flow,depth,InunArea_m2,CatchArea_m2,InunRatio\n");
    const float none = -9999.0;
    for (int i = 0; i < nfc; i++) {
        const int at = last_index(ids, nfc, ids[i]);
        const double d = depth[at];
        const float wet = area[at] > 0 ? area[at] : none;
        const float whole = carea[i];
        float ratio = none;
        if (wet != none && whole != none) ratio = wet / whole;
        fprintf(f, "%d,%.6f,%.6f,%.6f,%.6f,%.6f\n", ids[i], flow[i], d, wet, whole, ratio);
    }
    fclose(f);
    return 0;
}
