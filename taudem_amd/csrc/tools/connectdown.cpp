// connectdown -p p -w w -ad8 ad8 -o outlets -od movedoutlets [-d movedist] [-olyr n] [-odlyr n]
// (flag surface of src/ConnectDownmn.cpp:53-174; there is no simple form).  The layer options are accepted and ignored.
#include "cli_common.hpp"

static void usage() {
    printf("Incorrect input.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, wfile, ad8file, outlets, outletlyr, moved, movedlyr;
    int movedist = 10;
    if (argc < 10) {
        printf("No simple use case for this function.\n");
        usage();
    }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-p")) { if (!a.value(pfile)) usage(); }
        else if (a.is("-w")) { if (!a.value(wfile)) usage(); }
        else if (a.is("-ad8")) { if (!a.value(ad8file)) usage(); }
        else if (a.is("-o")) { if (!a.value(outlets)) usage(); }
        else if (a.is("-olyr")) { if (!a.value(outletlyr)) usage(); }
        else if (a.is("-od")) { if (!a.value(moved)) usage(); }
        else if (a.is("-odlyr")) { if (!a.value(movedlyr)) usage(); }
        else if (a.is("-d")) { if (!a.value(movedist)) usage(); }
        else usage();
    }
    const int err = tdx_tool_connectdown(pfile.c_str(), wfile.c_str(), ad8file.c_str(), outlets.c_str(), outletlyr.c_str(), moved.c_str(), movedlyr.c_str(), movedist);
    if (err == 4) { fflush(stdout); return 4; }   // MPI_Abort(MCW, 4): a raster that does not match w
    if (err == TDX_ERR_ARG) return 2;             // an output this build cannot write, or an id outside 0 .. TDX_CONNECTDOWN_MAX_ID: said on stderr
    return cli::finish("Move down", err);
}
