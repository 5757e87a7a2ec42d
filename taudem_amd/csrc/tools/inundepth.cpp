// inundepth -hand h -catch c [-mask m] -fc forecast.csv -hp table -inun map.tif [-depth depth.csv]   (flag surface of src/InunDepthmn.cpp:65-167)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Use with specific file names:\n %s -hand <handfile>\n", prog);
    printf("-catch <catchfile> -mask <maskfile> \n");
    printf("-fc <forecastfile> -hp <hydropropertyfile> \n");
    printf("-inun <outputinundationfile> \n");
    printf("-depth <outputdepthfile> \n");
    printf("<handfile> is the name of the input hand raster file - required file.\n");
    printf("<catchfile> is the name of the input catchment COMID raster file - required file.\n");
    printf("<maskfile> is the name of the mask raster file - optional file, e.g. waterbody.\n");
    printf("<forecastfile> is the name of the inundation forecast CSV file - required file, with columns: id, flow.\n");
    printf("<hydropropertyfile> is the name of the hydro property text file - required file.\n");
    printf("<outputinundationfile> is the name of the output inundation raster file - required file.\n");
    printf("<outputdepthfile> is the name of the output inundation depth text/CSV file - optional file.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string handfile, catchfile, maskfile, fcfile, hpfile, mapfile, depthfile;
    bool has_mask = false, has_depth = false;
    if (argc < 5) usage(argv[0]);
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-hand")) { if (!a.value(handfile)) usage(argv[0]); }
        else if (a.is("-catch")) { if (!a.value(catchfile)) usage(argv[0]); }
        else if (a.is("-mask")) { if (!a.value(maskfile)) usage(argv[0]); has_mask = true; }
        else if (a.is("-fc")) { if (!a.value(fcfile)) usage(argv[0]); }
        else if (a.is("-hp")) { if (!a.value(hpfile)) usage(argv[0]); }
        else if (a.is("-inun")) { if (!a.value(mapfile)) usage(argv[0]); }
        else if (a.is("-depth")) { if (!a.value(depthfile)) usage(argv[0]); has_depth = true; }
        else usage(argv[0]);
    }
    const int err = tdx_tool_inundepth(handfile.c_str(), catchfile.c_str(), has_mask ? maskfile.c_str() : nullptr, fcfile.c_str(), hpfile.c_str(), mapfile.c_str(),
                                       has_depth ? depthfile.c_str() : nullptr);
    return cli::finish("Inundation Depth Generation", err);
}
