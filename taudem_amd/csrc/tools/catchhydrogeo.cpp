// catchhydrogeo -hand h -catch c -catchlist l -slp s -h stages -table out   (flag surface of src/CatchHydroGeomn.cpp:62-138)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Incorrect input.\n");
    printf("Use with specific file names:\n %s -hand <handfile>\n", prog);
    printf("-catch <catchfile> -catchlist <catchidlistfile> -slp <slpfile> -h <hfile> -table <hpfile> \n");
    printf("<handfile> is the name of the input hand raster file.\n");
    printf("<catchfile> is the name of the input catchment raster file.\n");
    printf("<catchidlistfile> is the name of the input catchment id list CSV file. This file has at least 3 columns: catchment id, catchment slope, catchment length. "
           "Optionally, a 4th column for Manning's n can be provided.\n");
    printf("<slpfile> is the name of the input D-inf slope raster file.\n");
    printf("<hfile> is the name of the input stage table text file.\n");
    printf("<hpfile> is the name of the output hydraulic property text file.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string handfile, catchfile, listfile, slpfile, hfile, hpfile;
    if (argc < 6) usage(argv[0]);
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-hand")) { if (!a.value(handfile)) usage(argv[0]); }
        else if (a.is("-catch")) { if (!a.value(catchfile)) usage(argv[0]); }
        else if (a.is("-catchlist")) { if (!a.value(listfile)) usage(argv[0]); }
        else if (a.is("-slp")) { if (!a.value(slpfile)) usage(argv[0]); }
        else if (a.is("-h")) { if (!a.value(hfile)) usage(argv[0]); }
        else if (a.is("-table")) { if (!a.value(hpfile)) usage(argv[0]); }
        else usage(argv[0]);
    }
    const int err = tdx_tool_catchhydrogeo(handfile.c_str(), catchfile.c_str(), listfile.c_str(), slpfile.c_str(), hfile.c_str(), hpfile.c_str());
    return cli::finish("Catchment Hydraulic Property", err);
}
