// slopeavedown -p p -fel fel -slpd slpd [-dn distance]   (flag surface of src/SlopeAveDownmn.cpp:49-140; default -dn 50)
// A -dn that is negative, not finite or not a number is refused with a non-zero exit.  The number of passes is not capped.
#include <cmath>

#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple Usage:\n %s <basefilename>\n", prog);
    printf("Usage with specific file names:\n %s -p <pfile>\n", prog);
    printf("-fel <felfile> -slpd <slpdfile> -dn <dn>\n");
    printf("<basefilename> is the name of the base digital elevation model\n");
    printf("<pfile> is the d8 flow direction input file.\n");
    printf("<felfile> is the pit filled or carved elevation input file.\n");
    printf("<slpdfile> is the D8 slope distance averaged output file.\n");
    printf("<dn> is the optional user selected downslope distance (default 50).\n");
    printf("With the simple form the suffixes p, fel and slpd are inserted before the extension of <basefilename>.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, felfile, slpdfile, dntext;
    double dn = 50.0;   // src/SlopeAveDownmn.cpp:53
    if (argc < 2) { printf("Error: To run this program, use either the Simple Usage option or\nthe Usage with Specific file names option\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-slpd")) { if (!a.value(slpdfile)) usage(argv[0]); }
        else if (a.is("-dn")) {
            if (!a.value(dntext)) usage(argv[0]);
            char* end = nullptr;
            dn = strtod(dntext.c_str(), &end);
            if (end == dntext.c_str() || *end != '\0' || !std::isfinite(dn) || dn < 0.0) {
                fprintf(stderr, "slopeavedown: -dn must be a finite distance that is not negative (got '%s')\n", dntext.c_str());
                return 2;
            }
        }
        else usage(argv[0]);
    }
    if (argc == 2) { felfile = cli::nameadd(argv[1], "fel"); pfile = cli::nameadd(argv[1], "p"); slpdfile = cli::nameadd(argv[1], "slpd"); }
    const int err = tdx_tool_slopeavedown(pfile.c_str(), felfile.c_str(), slpdfile.c_str(), dn);
    return cli::finish("Slope average down", err);
}
