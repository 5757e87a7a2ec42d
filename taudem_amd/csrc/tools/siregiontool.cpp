// siregiontool --dem <dem> --parreg <region grid> --att <region table> [--parreg-in <region grid> | --shp <polygon layer> [--shp-att-name ID]]
//              [--att-tmin 2.708] [--att-tmax 2.708] [--att-cmin 0.0] [--att-cmax 0.25] [--att-phimin 30.0] [--att-phimax 45.0] [--att-soildens 2000.0] [--gpus N]
// (the toolbox step "Create Parameter Region Grid": the flags of pyfiles/SIRegionTool.py; like the script it ends with "Region computation successful."
// or with "Region computation failed.", the reason and exit status 1; the parameter texts go into the table as they were given)
#include "cli_common.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string dem, parreg, att, parreg_in, shp, shp_att = "ID";
    std::string par[7] = {"2.708", "2.708", "0.0", "0.25", "30.0", "45.0", "2000.0"};
    const char* par_flags[7] = {"--att-tmin", "--att-tmax", "--att-cmin", "--att-cmax", "--att-phimin", "--att-phimax", "--att-soildens"};
    bool ok = true;
    for (int i = 1; ok && i < argc; i += 2) {
        std::string flag = argv[i], value;
        const size_t eq = flag.find('=');
        if (eq != std::string::npos) { value = flag.substr(eq + 1); flag.resize(eq); i--; }   // --flag=value, as argparse takes it
        else if (i + 1 < argc) value = argv[i + 1];
        else { ok = false; break; }
        std::string* dst = flag == "--dem" ? &dem : flag == "--parreg" ? &parreg : flag == "--att" ? &att : flag == "--parreg-in" ? &parreg_in : flag == "--shp" ? &shp
                           : flag == "--shp-att-name" ? &shp_att : nullptr;
        for (int k = 0; k < 7 && !dst; k++)
            if (flag == par_flags[k]) dst = &par[k];
        if (!dst) ok = false;
        else *dst = value;
    }
    if (!ok || dem.empty() || parreg.empty() || att.empty()) {
        printf("Usage: %s --dem <dem> --parreg <output region grid> --att <output region table> [--parreg-in <region grid> | --shp <polygon layer: .shp, .json or "
               ".geojson> [--shp-att-name <field, default ID>]] [--att-tmin v] [--att-tmax v] [--att-cmin v] [--att-cmax v] [--att-phimin v] [--att-phimax v] "
               "[--att-soildens v] [--gpus N]\n", argv[0]);
        return 0;
    }
    const char* texts[7];
    for (int k = 0; k < 7; k++) texts[k] = par[k].c_str();
    const int err = tdx_tool_siregiontool(dem.c_str(), parreg.c_str(), att.c_str(), parreg_in.c_str(), shp.c_str(), shp_att.c_str(), texts);
    if (err == 0) {
        printf("Region computation successful.\n");
        return 0;
    }
    printf("Region computation failed.\n%s\n", tdx_last_error(nullptr));
    return 1;
}
