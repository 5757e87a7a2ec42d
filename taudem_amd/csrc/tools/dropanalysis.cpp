// dropanalysis -ad8 a -p p -fel f -ssa s -o outlets -drp table [-par min max nthresh steptype] [-lyrname n] [-lyrno i]
// (flag surface of src/DropAnalysismn.cpp:53-207; defaults 5 500 10 0)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("\nUse with specific file names:\n %s -slp <slopefile>\n", prog);
    printf("-ad8 <ad8file> -p <dirfile> -fel <elevfile> -ssa <ssafile> -o <outletsshapefile>\n");
    printf("-drp <dropfile> [-par <min> <max> <nthresh> <steptype>] \n");
    printf("<ad8file> is the name of the input contributing area file used in calculations of drainage density. \n");
    printf("<dirfile> is the name of the input D8 flow directions file.\n");
    printf("<elevfile> is the name of the input elevation file.\n");
    printf("<ssafile> is the name of the accumulated stream source file.  This needs to have the property that it is\n");
    printf("monotonically increasing downstream along the D8 flow directions.\n");
    printf("<outletsshapefile> is the name of the shapefile containing input outlets.\n");
    printf("<dropfile> a text file for drop analysis tabular output.\n");
    printf("<min> Lower bound of range used to search for optimum threshold.\n");
    printf("<max> Upper bound of range used to search for optimum threshold.\n");
    printf("<nthresh> Number of thresholds used to search for optimum threshold.\n");
    printf("<steptype> Type of threshold step to be used (0=log, 1=arithmetic).\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string areafile, dirfile, elevfile, ssafile, dropfile, datasrc, lyrname;
    float threshmin = 5, threshmax = 500, threshopt = 0;
    int nthresh = 10, steptype = 0, uselyrname = 0, lyrno = 0;
    if (argc < 2) usage(argv[0]);
    if (argc == 2) {
        printf("No simple use option for this function because an outlets file is needed.\n");
        usage(argv[0]);
    }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-ad8")) { if (!a.value(areafile)) usage(argv[0]); }
        else if (a.is("-p")) { if (!a.value(dirfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(elevfile)) usage(argv[0]); }
        else if (a.is("-ssa")) { if (!a.value(ssafile)) usage(argv[0]); }
        else if (a.is("-o")) { if (!a.value(datasrc)) usage(argv[0]); }
        else if (a.is("-lyrno")) { if (!a.value(lyrno)) usage(argv[0]); }
        else if (a.is("-lyrname")) { if (!a.value(lyrname)) usage(argv[0]); uselyrname = 1; }
        else if (a.is("-drp")) { if (!a.value(dropfile)) usage(argv[0]); }
        else if (a.is("-par")) {
            if (a.argc <= a.i + 4) usage(argv[0]);
            sscanf(a.argv[a.i + 1], "%f", &threshmin);
            sscanf(a.argv[a.i + 2], "%f", &threshmax);
            sscanf(a.argv[a.i + 3], "%d", &nthresh);
            sscanf(a.argv[a.i + 4], "%d", &steptype);
            a.i += 5;
        }
        else usage(argv[0]);
    }
    if (datasrc.empty()) {   // the reference reads an uninitialised name here and fails to open it
        printf("dropanalysis: -o <outletsshapefile> is required\n");
        usage(argv[0]);
    }
    const int err = tdx_tool_dropanalysis(areafile.c_str(), dirfile.c_str(), elevfile.c_str(), ssafile.c_str(), dropfile.c_str(), datasrc.c_str(), lyrname.c_str(), uselyrname,
                                          lyrno, threshmin, threshmax, nthresh, steptype, &threshopt);
    return cli::finish("Drop Analysis", err);
}
