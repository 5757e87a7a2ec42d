#include "region_table.hpp"

#include <cctype>
#include <cstdio>
#include <cstdlib>

namespace regions {

const char* const kTableHeader = "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens";

bool write_table(const std::string& path, const int32_t* ids, int32_t n_ids, const char* const* seven_texts, std::string& err) {
    std::string text = std::string(kTableHeader) + "\n";
    for (int32_t k = 0; k < n_ids; k++) {
        text += std::to_string(ids[k]);
        for (int j = 0; j < 7; j++) { text += ","; text += seven_texts[j]; }
        text += "\n";
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { err = "cannot write " + path; return false; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { err = "cannot write " + path; return false; }
    return true;
}

bool attribute_values(const tdx::PolygonLayer& layer, const std::string& field, std::vector<int32_t>& values, std::string& err) {
    std::string up = field;
    for (char& c : up) c = char(toupper((unsigned char)c));
    if (up == "FID") { err = "the field FID is the record number, not an attribute: name a field that holds the region ids"; return false; }
    const int k = layer.field_index(field);
    if (k < 0) { err = "the polygon layer has no field " + field; return false; }
    values.clear();
    for (size_t i = 0; i < layer.values.size(); i++) {
        std::string t = size_t(k) < layer.values[i].size() ? layer.values[i][size_t(k)] : std::string();
        const size_t a = t.find_first_not_of(" \t\0", 0, 3), b = t.find_last_not_of(" \t\0", std::string::npos, 3);
        t = a == std::string::npos ? std::string() : t.substr(a, b - a + 1);
        const std::string who = "feature " + std::to_string(i) + ": " + field;
        if (t.empty() || t.find_first_not_of('*') == std::string::npos) { err = who + " is null"; return false; }
        // an integer: a sign, digits, and at most a fraction of zeros (what a Real column holds for a whole number)
        size_t p = (t[0] == '-' || t[0] == '+') ? 1 : 0, d0 = p;
        while (p < t.size() && isdigit((unsigned char)t[p])) p++;
        bool whole = p > d0 && p - d0 <= 18;
        if (whole && p < t.size()) {
            whole = t[p] == '.';
            for (size_t q = p + 1; whole && q < t.size(); q++) whole = t[q] == '0';
        }
        if (!whole) { err = who + " = " + t + " is not an integer"; return false; }
        const long long v = strtoll(t.c_str(), nullptr, 10);
        if (v < 1 || v > 32767) { err = who + " = " + std::to_string(v) + " is outside 1 .. 32767"; return false; }
        values.push_back(int32_t(v));
    }
    return true;
}

}  // namespace regions
