// gagewatershed -p p -o outlets -gw gw [-id idfile] [-lyrname n] [-lyrno i]   (flag surface of src/gagewatershedmn.cpp:44-160)
// -upid is recognised and refused: the reference's upstream-id file lists nodata neighbours in queue order, which depends on the schedule.
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Usage:\n %s -p <pfile> -o <outletshape> -gw <gagewatershed> [-id <idfile>]\n", prog);
    printf("<pfile> is the name of the input D8 flow direction grid file.\n");
    printf("<outletshape> is the name of the input outlet shapefile.\n");
    printf("<gagewatershed> is the output gagewatershed grid file.\n");
    printf("<idfile> is optional output text file giving watershed downslope connectivity.\n\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, wfile, datasrc, lyrname, idfile, upidfile;
    int uselyrname = 0, lyrno = 0, writeid = 0, writeupid = 0;
    if (argc <= 2) usage(argv[0]);
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-o")) { if (!a.value(datasrc)) usage(argv[0]); }
        else if (a.is("-lyrno")) { if (!a.value(lyrno)) usage(argv[0]); }
        else if (a.is("-lyrname")) { if (!a.value(lyrname)) usage(argv[0]); uselyrname = 1; }
        else if (a.is("-gw")) { if (!a.value(wfile)) usage(argv[0]); }
        else if (a.is("-id")) { if (!a.value(idfile)) usage(argv[0]); writeid = 1; }
        else if (a.is("-upid")) { if (!a.value(upidfile)) usage(argv[0]); writeupid = 1; }
        else usage(argv[0]);
    }
    if (writeupid) {
        fprintf(stderr, "gagewatershed: -upid is not supported: the reference writes that file in the order its queue visits cells, which no other schedule "
                        "reproduces\n");
        return 2;
    }
    const int err = tdx_tool_gagewatershed(pfile.c_str(), wfile.c_str(), datasrc.c_str(), lyrname.c_str(), uselyrname, lyrno, idfile.c_str(), writeid, writeupid,
                                           upidfile.c_str());
    return cli::finish("Gage watershed", err);
}
