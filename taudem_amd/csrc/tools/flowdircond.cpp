// flowdircond -p p -z z -zfdc zfdc   (flag surface of src/flowdirconditionmn.cpp:55-130)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple Usage:\n %s <basefilename>\n", prog);
    printf("Usage with specific file names:\n %s -p <pfile>\n", prog);
    printf("-z <zfile> -zfdc <zfdcfile>\n");
    printf("<basefilename> is the name of the base digital elevation model\n");
    printf("<pfile> is the d8 flow direction input file.\n");
    printf("<zfile> is the elevation input file.\n");
    printf("<zfdcfile> is the flow direction conditioned elevation output file.\n");
    printf("With the simple form the suffixes p, z and zfdc are inserted before the extension of <basefilename>.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, zfile, zfdcfile;
    if (argc < 2) { printf("Error: To run this program, use either the Simple Usage option or\nthe Usage with Specific file names option\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-z")) { if (!a.value(zfile)) usage(argv[0]); }
        else if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-zfdc")) { if (!a.value(zfdcfile)) usage(argv[0]); }
        else usage(argv[0]);
    }
    if (argc == 2) { zfile = cli::nameadd(argv[1], "z"); pfile = cli::nameadd(argv[1], "p"); zfdcfile = cli::nameadd(argv[1], "zfdc"); }
    const int err = tdx_tool_flowdircond(pfile.c_str(), zfile.c_str(), zfdcfile.c_str());
    return cli::finish("Flow direction conditioning", err);
}
