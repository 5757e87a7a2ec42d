// peukerdouglas -fel fel -ss ss [-par weightMiddle weightSide weightDiagonal]   (flag surface of src/PeukerDouglasmn.cpp:53-128; defaults 0.4 0.1 0.05)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple Use:\n %s <basefilename>\n", prog);
    printf("Use with specific file names:\n %s -fel <elevationfile>\n", prog);
    printf("-ss <streamsource> [-par <weightMiddle> <weightSide> <weightDiagonal>]\n");
    printf("<basefilename> is the name of the base digital elevation model without suffixes for simple input. 'fel' will be appended. \n");
    printf("<elevationfile> is the name of the elevation input file.\n");
    printf("<streamsource> is the name of the stream source file output.\n");
    printf("The elevation input is smoothed by averaging using the center and eight surrounding grid cells.\n");
    printf("<weightMiddle> is the weight given to the center cell in the smoothing of the input elevations.\n");
    printf("<weightSide> is the weight given to the 4 side cells in the smoothing of the input elevations.\n");
    printf("<weightDiagonal> is the weight given to the 4 diagonal cells in the smoothing of the input elevations.\n");
    printf("Default weights are 0.4 0.1 0.05 if -par is not specified.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string felfile, ssfile;
    float p[3] = {0.4f, 0.1f, 0.05f};
    if (argc < 2) usage(argv[0]);
    if (argc == 2) { felfile = cli::nameadd(argv[1], "fel"); ssfile = cli::nameadd(argv[1], "ss"); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-ss")) { if (!a.value(ssfile)) usage(argv[0]); }
        else if (a.is("-par")) {
            if (a.argc <= a.i + 3) usage(argv[0]);
            sscanf(a.argv[a.i + 1], "%f", &p[0]);
            sscanf(a.argv[a.i + 2], "%f", &p[1]);
            sscanf(a.argv[a.i + 3], "%f", &p[2]);
            a.i += 4;
        }
        else usage(argv[0]);
    }
    const int err = tdx_tool_peukerdouglas(felfile.c_str(), ssfile.c_str(), p);
    if (err != 0 && !cli::is_abort_code(err)) { printf("Peuker Douglas Error %d\n", err); return 0; }
    return cli::finish("Peuker Douglas", err);
}
